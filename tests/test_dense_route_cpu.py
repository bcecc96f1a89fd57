"""Host-side dispatch of the dense stages (gsn_amd/_dense.py) on CPU tensors -- no kernel runs: when a product goes to the fp16x3 kernel
(_f16x3_takes, the one statement of that rule, at its edges under the default switches) and how a gsn_block descriptor array is filled."""
import pytest
import torch

from gsn_amd import _dense, flags

M_BIG = 128 * 64              # 64 row tiles: the tile count is past the threshold for every n_out > 128 below


@pytest.fixture(autouse=True)
def default_flags(monkeypatch):
    for name, value in (("LINEAR_F16X3", True), ("LINEAR_F16X3_STATS", True), ("LINEAR_F16X3_MIN_N", 128), ("LINEAR_F16X3_MIN_TILES", 96)):
        monkeypatch.setattr(flags, name, value)


def takes(m_rows=M_BIG, n_out=256, widths=(128, 12), **kw):
    return bool(_dense._f16x3_takes(m_rows, n_out, list(widths), **kw))


def test_n_out_edge():
    assert not takes(n_out=128)
    assert takes(n_out=129)


def test_tile_count_edge():
    # n_out 256: two column tiles; 48 row tiles make 96 tiles (not taken), one more row makes 49 x 2 = 98
    assert not takes(m_rows=48 * 128, n_out=256)
    assert takes(m_rows=48 * 128 + 1, n_out=256)
    assert not takes(m_rows=0)


def test_blocks_widths_alignment_gather():
    assert not takes(widths=(128, 6))                 # a width that is not a multiple of 4
    assert not takes(aligned=False)                   # a block that is not 16-byte aligned
    assert not takes(direct=False)                    # a block gathered through an index
    assert takes(widths=(128, 8, 4))


def test_stats_case():
    assert takes(stats=True)                                         # no BN vectors, identity activation, n_out % 4 == 0
    assert not takes(stats=True, bn=True)
    assert not takes(stats=True, act=1)
    assert not takes(stats=True, n_out=258) and takes(n_out=258)     # (n_out % 4 binds the statistics epilogue only)
    assert takes(bn=True, act=1)                                     # (BN vectors / an activation in the plain epilogue: taken)


def test_switches_and_no_output():
    assert not takes(out=False)
    flags.LINEAR_F16X3_STATS = False
    assert not takes(stats=True) and takes()
    flags.LINEAR_F16X3 = False
    assert not takes()


def test_block_array_fills_descriptors_and_keeps_what_they_point_at():
    x = torch.zeros(5, 8)
    h = torch.zeros(3, 4, dtype=torch.float64)           # converted to fp32: the copy is what the descriptor points at
    i32 = torch.arange(5, dtype=torch.int32)
    i64 = torch.arange(5, dtype=torch.int64)
    keep = []
    arr = _dense._block_array([(x, i32), (x, i64), (h, None)], keep)
    assert [arr[b].width for b in range(3)] == [8, 8, 4]
    assert arr[0].data == x.data_ptr() and arr[0].idx32 == i32.data_ptr() and arr[0].idx is None
    assert arr[1].idx == i64.data_ptr() and arr[1].idx32 is None
    assert arr[2].idx is None and arr[2].idx32 is None
    h32 = [t for t in keep if isinstance(t, torch.Tensor) and t.dtype is torch.float32 and t.shape == (3, 4)]
    assert len(h32) == 1 and arr[2].data == h32[0].data_ptr()
    assert any(t is arr for t in keep)
    only = _dense._block_array([(x, i32), (h, None)], [], widths_only=True)
    assert [only[b].width for b in range(2)] == [8, 4] and only[0].idx32 is None
