"""The host side of the key path of gsn_amd.step.CountLayerStep (gsn_count_layer_step_keys_hip): the byte -> fragment table the layer kernel
expands its edge-level operand rows from, the node dictionary's tuple order against the key function, and the gate."""
import ctypes
import itertools

import numpy as np
import pytest


def test_byte_table_holds_the_bits_of_every_byte_as_fp16_ones():
    from gsn_amd import _abi
    tab = np.zeros((256, 8), dtype=np.uint16)
    assert _abi.lib().gsn_layer_keys_byte_table(tab.ctypes.data_as(ctypes.c_void_p)) == 0
    want = np.zeros((256, 8), dtype=np.float16)
    for b in range(256):
        for j in range(8):
            want[b, j] = 1.0 if (b >> j) & 1 else 0.0
    assert np.array_equal(tab, want.view(np.uint16))
    assert np.array_equal(tab.view(np.float16).astype(np.int64) @ (1 << np.arange(8)), np.arange(256))      # (every byte comes back from its row)


@pytest.mark.parametrize("n_classes,clamp", [([28], True), ([28], False), ([7, 4], True), ([7, 4], False), ([3, 2, 5, 2], False), ([1], False)])
def test_dictionary_tuples_are_numbered_by_the_key_function(n_classes, clamp):
    from gsn_amd.step import node_dict_tuples, node_key, node_key_radices
    radices = node_key_radices(n_classes, clamp)
    assert radices == [c + (0 if clamp else 1) for c in n_classes]
    tuples = node_dict_tuples(n_classes, clamp)
    assert tuples.shape == (int(np.prod(radices)), len(n_classes))
    assert tuples.tolist() == [list(t) for t in itertools.product(*[range(r) for r in radices])]       # column 0 most significant
    # row k holds the tuple whose key is k -- also when its "none" digits are written as any other code outside the classes
    assert np.array_equal(node_key(tuples, n_classes, clamp), np.arange(tuples.shape[0]))
    if not clamp:
        wild = np.where(tuples == np.asarray(n_classes)[None, :], -3, tuples)
        assert np.array_equal(node_key(wild, n_classes, clamp), np.arange(tuples.shape[0]))
        wild = np.where(tuples == np.asarray(n_classes)[None, :], 1000, tuples)
        assert np.array_equal(node_key(wild, n_classes, clamp), np.arange(tuples.shape[0]))
    else:
        over = tuples + (tuples == np.asarray(n_classes)[None, :] - 1) * 9                               # codes above the last class: clamped to it
        assert np.array_equal(node_key(over, n_classes, clamp), np.arange(tuples.shape[0]))
        assert np.array_equal(node_key(np.full((1, len(n_classes)), -5), n_classes, clamp), [0])


def test_gate_is_a_dictionary_of_at_most_256_rows():
    from gsn_amd.step import keys_path_ok
    assert keys_path_ok([28], True) and keys_path_ok([28], False)
    assert keys_path_ok([7, 4], False) and keys_path_ok([16, 16], True) and keys_path_ok([256], True)
    assert not keys_path_ok([16, 16], False) and not keys_path_ok([256], False)          # (the "none" digits count)
    assert not keys_path_ok([7, 7, 7], True) and not keys_path_ok([7, 7, 6], True) and not keys_path_ok([7, 7, 7], False)
    assert keys_path_ok([4, 4, 4, 4], True) and not keys_path_ok([4, 4, 4, 4], False)
