"""Keras ``fit`` on a tiny decoder-only language model: ``Embedding`` -> causal
``MultiHeadAttention`` -> ``Add`` -> ``LayerNormalization`` -> ``Dense`` -> ``Dense(vocab)``,
trained on synthetic next-token data with ``SparseCategoricalCrossentropy(from_logits=True,
ignore_class=0)``: token 0 is padding, and padded positions count neither in the loss nor in
its mean.  The ``[B, T, V]`` logits go to the fused softmax cross-entropy kernels as they are.
The strategy comes from the wrapper ``run()`` generates (or OneDevice when run directly).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
from _common import n  # noqa: E402

from cloud_amd import tf  # noqa: E402

VOCAB = n(4099, 61)
SEQ = n(64, 12)
DIM = 64
HEADS = 2
BATCH_SIZE = n(64, 16)
EPOCHS = n(4, 2)


def make_data(count, seed):
    """Sequences that step through the vocabulary by a per-sequence stride (1..3), so the next
    token follows from the last two; a random-length tail of every sequence is padding (0)."""
    r = np.random.RandomState(seed)
    start = r.randint(1, VOCAB, size=(count, 1))
    stride = r.randint(1, 4, size=(count, 1))
    tokens = 1 + (start + stride * np.arange(SEQ + 1)[None, :]) % (VOCAB - 1)
    length = r.randint(SEQ // 2, SEQ + 2, size=(count, 1))
    tokens = np.where(np.arange(SEQ + 1)[None, :] < length, tokens, 0).astype(np.int64)
    return tokens[:, :-1], tokens[:, 1:]


x_train, y_train = make_data(n(8192, 256), 0)
x_test, y_test = make_data(n(1024, 64), 1)

inp = tf.keras.Input(shape=(SEQ,))
x = tf.keras.layers.Embedding(VOCAB, DIM)(inp)
a = tf.keras.layers.MultiHeadAttention(HEADS, DIM // HEADS, use_causal_mask=True)([x, x])
x = tf.keras.layers.Add()([x, a])
x = tf.keras.layers.LayerNormalization()(x)
x = tf.keras.layers.Dense(4 * DIM, activation="relu")(x)
out = tf.keras.layers.Dense(VOCAB)(x)
model = tf.keras.Model(inp, out)
model.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True, ignore_class=0),
              optimizer=tf.keras.optimizers.Adam(3e-3), metrics=["accuracy"])

hist = model.fit(x_train, y_train, batch_size=BATCH_SIZE, epochs=EPOCHS)
loss, acc = model.evaluate(x_test, y_test, batch_size=BATCH_SIZE, verbose=0)
print("RESULT fit loss={:.4f} first_loss={:.4f} eval_loss={:.4f} eval_acc={:.4f}".format(
    hist.history["loss"][-1], hist.history["loss"][0], loss, acc))
