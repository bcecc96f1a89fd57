"""Host side of training on padded batches, no GPU needed: the row-bounded BatchNorm and counted-loss entries exist in the
built library with the argument types gsn_amd._abi declares, the bound object validates what it is given, and the public entry points refuse
what they cannot take before anything is launched."""
import ctypes
import types

import pytest
import torch

from gsn_amd import _abi

NEW = ("gsn_bn_finalize_bounded_scratch_bytes", "gsn_bn_finalize_bounded_hip", "gsn_bn_act_bwd_from_h_bounded_hip",
       "gsn_masked_loss_fwd_counted_hip", "gsn_masked_loss_bwd_counted_hip")


def test_new_symbols_are_exported_with_the_declared_argtypes():
    L = _abi.lib()
    raw = ctypes.CDLL(_abi.LIB_PATH)
    i64, vp, dbl, ci = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    want = {
        "gsn_bn_finalize_bounded_scratch_bytes": (i64, [i64]),
        "gsn_bn_finalize_bounded_hip": (ci, [i64, i64, dbl, dbl, vp, vp, vp, vp, i64] + [vp] * 11),
        "gsn_bn_act_bwd_from_h_bounded_hip": (ci, [i64, i64] + [vp] * 6 + [ci, ci] + [vp] * 5 + [i64, vp]),
        "gsn_masked_loss_fwd_counted_hip": (ci, [ci, i64, i64] + [vp] * 6 + [i64, vp]),
        "gsn_masked_loss_bwd_counted_hip": (ci, [ci, i64, i64] + [vp] * 7),
    }
    for name in NEW:
        assert hasattr(raw, name), name
        assert _abi.SIGNATURES[name] == want[name], name
        fn = getattr(L, name)
        assert fn.restype is want[name][0] and list(fn.argtypes) == want[name][1], name


def test_scratch_size_and_host_side_argument_checks():
    """fp64 [2][C] partial sums and one 4-byte ticket per 64 columns, rounded to 8 bytes; bad arguments are refused before any launch"""
    L = _abi.lib()
    assert L.gsn_bn_finalize_bounded_scratch_bytes(0) == 0
    for c, want in ((1, 16 + 8), (64, 1024 + 8), (65, 1040 + 8), (300, 4800 + 24)):
        assert L.gsn_bn_finalize_bounded_scratch_bytes(c) == want
    one = 16      # (a non-null pointer that is never dereferenced: every call below is refused on the host)
    assert L.gsn_bn_finalize_bounded_hip(4, 8, 1e-5, 0.1, one, one, None, None, 0, one, None, None, None, None, one, one, one, one, None, None) == -1
    assert b"gsn_bn_finalize_bounded_hip" in L.gsn_last_error()
    assert L.gsn_bn_finalize_bounded_hip(4, 8, 1e-5, 0.1, one, one, one, None, 3, one, None, None, None, None, one, one, one, one, None, None) == -1
    assert L.gsn_bn_act_bwd_from_h_bounded_hip(8, 4, one, one, one, one, one, one, 1, 0, one, one, None, None, None, 0, None) == -1
    assert L.gsn_bn_act_bwd_from_h_bounded_hip(8, 4, one, one, one, one, one, one, 0, 0, one, one, None, one, None, 0, None) == -1
    assert L.gsn_masked_loss_fwd_counted_hip(1, 4, 1, one, one, None, one, one, None, 0, None) == -1
    assert L.gsn_masked_loss_bwd_counted_hip(1, 4, 1, one, one, None, one, one, one, None) == -1


def test_row_bound_validates_dtype_device_and_shape():
    from gsn_amd._bound import RowBound
    from gsn_amd.loader import RowBound as exported, masked_training
    assert exported is RowBound and callable(masked_training)
    with pytest.raises(TypeError, match="n_valid"):
        RowBound(torch.zeros(1, dtype=torch.int64))                      # not on the GPU
    with pytest.raises(TypeError, match="n_valid"):
        RowBound(3)
    with pytest.raises(TypeError, match="n_valid"):
        RowBound(torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="n_valid"):
        RowBound(torch.zeros(2, dtype=torch.int64))


def test_masked_training_wants_a_padded_batch_and_leaves_nothing_open():
    from gsn_amd import _bound
    from gsn_amd.loader import masked_training
    with pytest.raises(TypeError, match="PaddedBatch"):
        with masked_training(types.SimpleNamespace(x=None)):
            pass
    assert not _bound.is_active()
    assert _bound.active("vertex", "nobody") is None
    _bound.refuse("nobody")                  # (no block open: nothing to refuse)


def test_padded_train_step_refuses_a_plain_loader_and_a_bad_loss():
    from gsn_amd.graphs import PaddedTrainStep
    with pytest.raises(TypeError, match="PaddedDataLoader"):
        PaddedTrainStep(torch.nn.Linear(2, 2), [1, 2, 3], "L1Loss", None)
    with pytest.raises(TypeError, match="PaddedDataLoader"):
        PaddedTrainStep(torch.nn.Linear(2, 2), types.SimpleNamespace(batch_size=4), "L1Loss", None)


def test_masked_loss_n_valid_type_errors():
    from gsn_amd import evaluation as ev
    y_hat, y = torch.zeros(4, 1), torch.zeros(4, 1)
    for bad in (3, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(1)):
        with pytest.raises(TypeError, match="int64 tensor of one element"):
            ev.masked_loss("L1Loss", y_hat, y, n_valid=bad)
        with pytest.raises(TypeError, match="int64 tensor of one element"):
            ev.MaskedLoss("L1Loss")(y_hat, y, n_valid=bad)
    # a well-typed n_valid passes the type check: what stops the call on a machine without a GPU is the GPU requirement, not a TypeError
    with pytest.raises(RuntimeError):
        ev.masked_loss("L1Loss", y_hat, y, n_valid=torch.zeros(1, dtype=torch.int64))
