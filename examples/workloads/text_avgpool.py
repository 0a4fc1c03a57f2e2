"""Keras ``fit`` on a bag-of-embeddings text classifier: ``Embedding`` ->
``GlobalAveragePooling1D`` -> ``Dense`` -> ``Dense(classes)``, trained on synthetic token
sequences: every class owns a slice of the vocabulary, and a sequence draws about half of its
tokens from its class's slice and the rest from the whole vocabulary, so the mean embedding
separates the classes within a few epochs.  On the GPU the pooling runs on the in-tree global
average kernel through the ``[B, 1, T, C]`` view of the embedded sequence.
The strategy comes from the wrapper ``run()`` generates (or OneDevice when run directly).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
from _common import n  # noqa: E402

from cloud_amd import tf  # noqa: E402

VOCAB = n(2000, 120)
SEQ = n(64, 16)
DIM = n(64, 16)
CLASSES = 4
BATCH_SIZE = n(64, 16)
EPOCHS = n(4, 4)


def make_data(count, seed):
    """Class k owns the tokens of ``[k * VOCAB / CLASSES, (k + 1) * VOCAB / CLASSES)``; each
    position holds a token of the label's slice with probability 1/2, else any token."""
    r = np.random.RandomState(seed)
    labels = r.randint(0, CLASSES, size=count)
    width = VOCAB // CLASSES
    own = labels[:, None] * width + r.randint(0, width, size=(count, SEQ))
    noise = r.randint(0, VOCAB, size=(count, SEQ))
    tokens = np.where(r.rand(count, SEQ) < 0.5, own, noise)
    return tokens.astype(np.int64), labels.astype(np.int64)


x_train, y_train = make_data(n(8192, 256), 0)
x_test, y_test = make_data(n(1024, 64), 1)

L = tf.keras.layers
model = tf.keras.Sequential([
    L.Embedding(VOCAB, DIM, input_shape=(SEQ,)),
    L.GlobalAveragePooling1D(),
    L.Dense(DIM, activation="relu"),
    L.Dense(CLASSES),
])
model.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.Adam(1e-2), metrics=["accuracy"])

hist = model.fit(x_train, y_train, batch_size=BATCH_SIZE, epochs=EPOCHS)
loss, acc = model.evaluate(x_test, y_test, batch_size=BATCH_SIZE, verbose=0)
print("RESULT fit loss={:.4f} first_loss={:.4f} eval_loss={:.4f} eval_acc={:.4f}".format(
    hist.history["loss"][-1], hist.history["loss"][0], loss, acc))
