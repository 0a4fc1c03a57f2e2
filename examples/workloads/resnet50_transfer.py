"""ResNet-50 transfer learning: a frozen base, a trainable GlobalAveragePooling -> Dropout ->
Dense head, validation every epoch and early stopping on ``val_loss`` -- the model section of the
reference's ``call_run_within_script_with_keras_fit.py`` / ``dogs_classification`` notebook on
``cloud_amd.tf``, with synthetic images and ``weights=None`` (no network).

``base_model.trainable = False`` means what it means in Keras: the base runs in inference mode
inside ``fit`` too (its BatchNorms use and keep their moving statistics), nothing of it is saved
for a backward pass, and on an MI355X every one of its BatchNorms runs in the epilogue of its
convolution.  Only the Dense kernel and bias train.

The default size is tiny (runs in seconds on a CPU); ``--image 224 --n 2048 --batch 64`` is the
reference's shape.  ``--weights PATH`` starts the base from a file written by
``Model.save_weights`` of a ``ResNet50(include_top=False)`` of the same input shape.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cloud_amd import tf  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", type=int, default=32)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--n", type=int, default=32, help="training images")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--weights", default=None, help="save_weights file for the base (default: random init)")
    a = ap.parse_args(argv)

    rng = np.random.default_rng(0)
    x = rng.random((a.n, a.image, a.image, 3), dtype=np.float32) * 255
    y = rng.integers(0, a.classes, a.n)
    ds = tf.data.Dataset.from_tensor_slices((x, y))
    ds = ds.map(lambda im, lb: (tf.keras.applications.resnet50.preprocess_input(im), lb))
    ds_train = ds.batch(a.batch, drop_remainder=True).prefetch(tf.data.AUTOTUNE)
    ds_val = ds_train.take(2)

    inputs = tf.keras.layers.Input(shape=(a.image, a.image, 3))
    base_model = tf.keras.applications.ResNet50(weights=a.weights, include_top=False, input_tensor=inputs)
    base_model.trainable = False
    h = tf.keras.layers.GlobalAveragePooling2D()(base_model.output)
    h = tf.keras.layers.Dropout(0.5)(h)
    outputs = tf.keras.layers.Dense(a.classes)(h)
    model = tf.keras.Model(inputs, outputs)
    model.compile(optimizer=tf.keras.optimizers.Adam(learning_rate=1e-2),
                  loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True), metrics=["accuracy"])
    model.summary()

    history = model.fit(ds_train, epochs=a.epochs, validation_data=ds_val, verbose=2,
                        callbacks=[tf.keras.callbacks.EarlyStopping(monitor="val_loss", patience=3)])
    loss, acc = model.evaluate(ds_val, verbose=0)
    print("RESULT resnet50_transfer trainable_weights={} epochs={} val_loss={:.4f} val_acc={:.3f}".format(
        len(model.trainable_weights), len(history.history["loss"]), loss, acc))


if __name__ == "__main__":
    main()
