"""Test helper next to philox_ref.py: the Bernoulli(0.5) masks of the dense coupling flows as the kernels draw them
(lbbnn_dense_layer_t::draw_masks, lbbnn_flow_dense_members): philox_bits4 of csrc/lbbnn_device.h on Philox stream
LBBNN_STREAM_MASK * 64 + layer id, counter = element index, word 0 = the forward draw, bit t = transform t."""
import numpy as np

from philox_ref import MASK, key_of, philox4x32_10

STREAM_MASK = 6            # LBBNN_STREAM_MASK (include/lbbnn.h)


def mask_bits(seed, offset, layer_id, I, T):
    """(T, I) float32 in {0, 1}: the mask of transform t at element i for the Philox state {seed, offset}."""
    k0, k1 = key_of(seed, offset)
    i = np.arange(I, dtype=np.uint64)
    x, _, _, _ = philox4x32_10(i & np.uint64(MASK), i >> np.uint64(32), np.zeros(I, np.uint64),
                               np.full(I, STREAM_MASK * 64 + (int(layer_id) & 63), np.uint64), k0, k1)
    t = np.arange(T, dtype=np.uint64)[:, None]
    return ((x[None, :] >> t) & np.uint64(1)).astype(np.float32)
