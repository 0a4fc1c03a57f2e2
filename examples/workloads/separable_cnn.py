"""Keras ``fit`` on a small separable-convolution image classifier (the MobileNet / Xception
building blocks): ``Conv2D`` stem -> ``SeparableConv2D`` + ``BatchNormalization`` blocks with one
stride-2 ``DepthwiseConv2D`` between them -> ``GlobalAveragePooling2D`` -> ``Dense``, trained on
synthetic textures (stripes at four orientations plus noise), which the 3x3 depthwise filters
separate within a few epochs.  On the GPU every convolution runs in-tree: the depthwise halves
on the streaming kernels of ``dwconv.hip``, the pointwise halves on the GEMM.
The strategy comes from the wrapper ``run()`` generates (or OneDevice when run directly).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
from _common import n  # noqa: E402

from cloud_amd import tf  # noqa: E402

SIZE = n(32, 12)
WIDTH = n(32, 8)
CLASSES = 4
BATCH_SIZE = n(64, 16)
EPOCHS = n(4, 4)


def make_data(count, seed):
    """Class k: stripes of period 4 along direction k (horizontal, vertical, the two diagonals)
    at a random phase, in three channels of random sign, plus Gaussian noise."""
    r = np.random.RandomState(seed)
    labels = r.randint(0, CLASSES, size=count)
    yy, xx = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing="ij")
    coord = np.stack([yy, xx, yy + xx, yy - xx])[labels]  # [count, SIZE, SIZE]
    phase = r.randint(0, 4, size=(count, 1, 1))
    stripes = np.where((coord + phase) % 4 < 2, 1.0, -1.0)
    sign = r.choice([-1.0, 1.0], size=(count, 1, 1, 3))
    x = stripes[..., None] * sign + 0.5 * r.randn(count, SIZE, SIZE, 3)
    return x.astype(np.float32), labels.astype(np.int64)


x_train, y_train = make_data(n(4096, 192), 0)
x_test, y_test = make_data(n(1024, 64), 1)

L = tf.keras.layers
model = tf.keras.Sequential([
    L.Conv2D(WIDTH, 3, padding="same", activation="relu", input_shape=(SIZE, SIZE, 3)),
    L.SeparableConv2D(WIDTH, 3, padding="same", use_bias=False),
    L.BatchNormalization(momentum=0.9),
    L.ReLU(),
    L.DepthwiseConv2D(3, strides=2, padding="same", activation="relu"),
    L.SeparableConv2D(2 * WIDTH, 3, padding="same", use_bias=False),
    L.BatchNormalization(momentum=0.9),
    L.ReLU(),
    L.SeparableConv2D(2 * WIDTH, 3, padding="same", activation="relu"),
    L.GlobalAveragePooling2D(),
    L.Dense(CLASSES),
])
model.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.Adam(3e-3), metrics=["accuracy"])

hist = model.fit(x_train, y_train, batch_size=BATCH_SIZE, epochs=EPOCHS)
loss, acc = model.evaluate(x_test, y_test, batch_size=BATCH_SIZE, verbose=0)
print("RESULT fit loss={:.4f} first_loss={:.4f} eval_loss={:.4f} eval_acc={:.4f}".format(
    hist.history["loss"][-1], hist.history["loss"][0], loss, acc))
