"""Every dispatch rung and pipeline state of csrc/propagate.hip, compared EXACTLY with an fp64 reference, each case stating the kernels it ran.

Which kernel a shape takes is read from the library itself: every launch site of propagate.hip notes what it launched and
``gsn_propagate_last_route()`` returns it ("relu_sum3<16,5,2,nt0,ext0,c1> grid=1;..."), so a moved threshold moves a case's route and fails here.
The report is thread-local and cleared by every entry point, and autograd runs the adjoints on its own thread: ``_Routes`` stands in for the
ctypes handle and reads the report right behind each propagate / CSR call, on the thread that made it.

Equality instead of a tolerance: every input (a, b, c, the self blocks, the upstream gradient) is k / 8 with k an integer in [-8, 8] and eps is
0.25 or 0.5.  A message element is then a multiple of 1/8 of magnitude <= 3, (1 + eps) * x a multiple of 1/32, and a sum over a segment of fewer
than 2^17 rows stays below 2^24 units: every fp32 sum and product in the kernels is exact whatever its order, and so is the fp64 reference cast
to fp32.  Outputs, gradients and g_eps (an fp64 sum cast once) must satisfy torch.equal; there is no ReLU-flip allowance because (a + b) + c is
exact -- 4 to 6 % of the pre-activations are exactly zero, which pins the kernels' ``pre > 0`` convention (the reference states it).
Concatenation blocks are drawn from the non-zero values so that a dropped row cannot hide.

Graphs: per-target in-degrees 0, 1, 2, 3, 4, 5, 8, 13, 16, 17 and 29 (around the four prefetched edges, the 4- and 16-row unrolls), one hub
holding a third of the edges, the out-degrees a permutation of the in-degrees (the node passes walk the source-sorted CSR), edge order a random
permutation.  "spread" tiles that list (E ~ 13 n: long segments), "sparse" holds it once among degrees 0..3 (E ~ 1.5 n).  Above 2 000 vertices
the hub stops at 2 048 edges: the CSR build restores a segment's order with an insertion sort and the sums must stay below 2^17 rows.
The cases of the pipe test run every lane group over ONE target; the capped cases here (fourth field of GSN_PROP_RS, third of GSN_PROP_CP,
and graphs of 3 * 2^18 + 5 713 vertices for the adjoints, whose cap is fixed) run three full steps and a partial one, so the rotated
registers are consumed.

What the table covers is every kernel instantiation the dispatch rules pick on their own (EVERY_KERNEL below spells them out), plus the
relu_sum3 mappings GSN_PROP_RS forces.  Deliberately without a case: instantiations that only GSN_PROP_LPR reaches (read once per process, so
a test cannot switch it) or only a forced GSN_PROP_CP mapping, and edge_split_sum / csr_graphs / segsum_prepare, which have their own tests.
``_segment_sum_cols`` copies a slice that is not 16-byte aligned, so the pointer half of the kernels' alignment test is reached through
``propagate`` on views that start one float into their storage (the misaligned_* cases)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPREAD = [0, 1, 2, 3, 4, 5, 8, 13, 16, 17, 29]
CSR_KERNELS = {"csr_small", "csr_zero", "csr_hist", "scan_tile_sums", "scan_tile_offsets", "scan_apply", "csr_fill", "csr_sort_segments"}
ROUTED = {"gsn_csr_build_hip", "gsn_propagate_fwd_hip", "gsn_propagate_self_fwd_hip", "gsn_segment_sum_rows_hip", "gsn_propagate_bwd_hip",
          "gsn_propagate_pad_bwd_hip", "gsn_propagate_bwd_fold_self_hip", "gsn_propagate_self_bwd_hip"}


class _Routes:
    """Stands in for the ctypes handle ``_abi.lib()`` returns: the route report is read behind every propagate / CSR entry point."""

    def __init__(self, real):
        self._real, self.log = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in ROUTED:
            return fn

        def call(*args):
            rc = fn(*args)
            text = self._real.gsn_propagate_last_route().decode()
            self.log.extend(x for x in text.split(";") if x)
            return rc
        return call

    def take(self):
        out, self.log = self.log, []
        return [_parse(x) for x in out]


def _parse(entry):
    m = re.fullmatch(r"(\S+) grid=(\d+)(?:x(\d+))?", entry)
    assert m, entry
    return m.group(1), int(m.group(2))


# ------------------------------------------------------------------------------------------------------------------
# graphs and inputs
# ------------------------------------------------------------------------------------------------------------------
def _degrees(n, profile, rng):
    if profile == "empty":
        return np.zeros(n, dtype=np.int64)
    base = np.array(SPREAD[-n:], dtype=np.int64)                  # (fewer than eleven vertices: the longest segments)
    if profile == "spread":
        deg = np.resize(base, n)
    else:
        deg = rng.integers(0, 4, n).astype(np.int64)
        deg[:base.size] = base
    if n > len(SPREAD):
        deg[len(SPREAD)] = 0
        deg[len(SPREAD)] = min(int(deg.sum()) // 2, 2048 if n > 2000 else (1 << 17) - 1)      # the hub: a third of all edges
    return deg


@functools.lru_cache(maxsize=None)
def _graph(n, profile, seed=0):
    """(edge_index [2, E] on the device: row 0 = source, row 1 = target; in-degrees; out-degrees)."""
    rng = np.random.default_rng(1000 * seed + n)
    indeg = rng.permutation(_degrees(n, profile, rng))
    outdeg = rng.permutation(indeg)
    tgt = np.repeat(np.arange(n), indeg)
    src = rng.permutation(np.repeat(np.arange(n), outdeg))
    order = rng.permutation(tgt.size)
    ei = torch.from_numpy(np.stack([src[order], tgt[order]]).astype(np.int64)).to(DEV)
    return ei, indeg, outdeg


def _dyadic(rows, width, gen, nonzero=False):
    if nonzero:
        k = torch.randint(1, 9, (rows, width), generator=gen, device=DEV) * (2 * torch.randint(0, 2, (rows, width), generator=gen, device=DEV) - 1)
    else:
        k = torch.randint(-8, 9, (rows, width), generator=gen, device=DEV)
    return k.to(torch.float64) / 8


# ------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------
def F(vec, lpr, maxc, ext=0, u4=1):
    return "propagate_fwd<%d,%d,%d,ext%d,u%d>" % (vec, lpr, maxc, ext, u4)


def RS(lpr, maxc, unr, nt=0, ext=0, c=1):
    return "relu_sum3<%d,%d,%d,nt%d,ext%d,c%d>" % (lpr, maxc, unr, nt, ext, c)


def CP(lpr, maxc, unr, ext=0):
    return "cat_pipe<%d,%d,%d,ext%d>" % (lpr, maxc, unr, ext)


WG = "segment_sum_wg"
E_GEN, E_CAT4, E_R4, E_R4P = "propagate_bwd_edge", "propagate_bwd_edge_cat4", "propagate_bwd_edge_relu4", "propagate_bwd_edge_relu4p"
N_GEN, N_E4, N_E4P, N_FOLD = "propagate_bwd_node", "propagate_bwd_node_edge4", "propagate_bwd_node_edge4p<fold0>", "propagate_bwd_node_edge4p<fold1>"
S_FLAT, S_GEN = "propagate_self_bwd_flat", "propagate_self_bwd"
CAT, RELU = 0, 1
CASES = []


def K(name, kind, widths, fwd, bwd=(), n=203, profile="spread", bpn=False, pads=(0, 0), selfs=(), eps=None, grads="", env=None, steady=None,
      grids=None, offset=0):
    """kind / widths (da, db, dc; 0 = no such block) / bpn / pads / selfs / eps: the call.  selfs: "a" (the gathered block itself), ("n", w) a
    per-node block, ("1", w) one row for every vertex.  grads: which of a b c e(ps) s(elf blocks) require a gradient.  env: (variable, value).
    fwd / bwd: the kernels the forward / the backward must report, in order.  steady: (phase, kernel, rows per workgroup, least number of full
    steps): a capped launch whose lane groups iterate.  grids: {kernel: grid} a launch that must have reached its cap.  offset: the fp32 inputs
    are contiguous views that start this many floats into their storage."""
    CASES.append(dict(name=name, call="propagate", kind=kind, widths=widths, fwd=list(fwd), bwd=list(bwd), n=n, profile=profile, bpn=bpn, pads=pads,
                      selfs=tuple(selfs), eps=eps, grads=grads, env=env, steady=steady, grids=grids or {}, offset=offset))


def S(name, n, width, fwd, col0=4, ld=None, profile="spread"):
    """layers._segment_sum_cols over rows [E, ld], columns col0 .. col0 + width."""
    CASES.append(dict(name=name, call="segsum", n=n, width=width, col0=col0, ld=ld or width + 8, fwd=list(fwd), bwd=[], profile=profile, env=None,
                      steady=None, grids={}, grads=""))


# --- segment_sum_wg_kernel: n <= 512 targets, E >= 8 n, one / two / four column passes; targets of 0 .. 3 rows leave waves idle
S("segwg_n1_d300", 1, 300, [WG])
S("segwg_n37_d4", 37, 4, [WG])
S("segwg_n37_d1024", 37, 1024, [WG])
S("segwg_n512_d300", 512, 300, [WG])
S("segwg_n513_is_cat_pipe", 513, 300, [CP(64, 2, 4)])
# (a slice that is not 16-byte aligned is copied by the Python side: the kernel sees an aligned pointer and an odd width)
S("segsum_col0_1_w7", 37, 7, [F(1, 16, 1)], col0=1, ld=12)

# --- relu_sum3_kernel, default mapping; the adjoints of the same shapes
K("rs3_d132_abc", RELU, (132, 132, 132), [RS(16, 5, 2)], [E_R4P, N_E4P], grads="abc")
K("rs3_d300_abc_fold", RELU, (300, 300, 300), [RS(16, 5, 1, ext=1)], [E_R4P, N_FOLD], selfs=("a",), eps=0.25, grads="abce")
K("rs3_d320_ab", RELU, (320, 320, 0), [RS(16, 5, 2, c=0)], [E_R4P, N_E4P], grads="ab")
K("rs3_d300_ac_self", RELU, (300, 0, 300), [RS(16, 5, 1, ext=1, c=0)], [E_R4P, N_E4P], selfs=(("n", 300),), eps=0.5, grads="ac")
K("rs3_d324_abc_outside_fold", RELU, (324, 324, 324), [RS(32, 3, 2, ext=1)], [E_R4, N_E4, S_FLAT], selfs=("a",), eps=0.25, grads="abce")
K("rs3_d384_ac", RELU, (384, 0, 384), [RS(32, 3, 4, c=0)], [E_R4, N_E4], grads="ac")
K("rs3_d384_abc_self", RELU, (384, 384, 384), [RS(32, 3, 2, ext=1)], selfs=(("n", 384),), eps=0.5)
K("rs3_d300_partial_wave", RELU, (300, 300, 300), [RS(16, 5, 2)], n=37, profile="sparse")
K("rs3_d300_n1", RELU, (300, 300, 0), [RS(16, 5, 2, c=0)], n=1)
# forced mappings, nontemporal loads off and on
for _l, _m in ((16, 5), (32, 3), (64, 2)):
    for _u in ((1, 2) if _l == 16 else (1, 2, 4)):
        for _nt in (0, 1):
            K("rs3_forced_%d_%d_nt%d" % (_l, _u, _nt), RELU, (300, 300, 300), [RS(_l, _m, _u, nt=_nt)], env=("GSN_PROP_RS", "%d,%d,%d" % (_l, _u, _nt)))
# the block cap: 203 targets against steps of 16 / 32 (16 lanes per target) and 8 / 16 (32 lanes)
for _b in (1, 2):
    K("rs3_cap%d_16lanes" % _b, RELU, (300, 300, 300), [RS(16, 5, 2)], env=("GSN_PROP_RS", "16,0,0,%d" % _b), steady=("fwd", "relu_sum3", 16, 3))
    K("rs3_cap%d_32lanes" % _b, RELU, (384, 384, 384), [RS(32, 3, 4)], env=("GSN_PROP_RS", "32,0,0,%d" % _b), steady=("fwd", "relu_sum3", 8, 3))
K("rs3_cap1_16lanes_self_b_only", RELU, (300, 300, 0), [RS(16, 5, 1, ext=1, c=0)], selfs=("a",), eps=0.5, env=("GSN_PROP_RS", "16,0,0,1"),
  steady=("fwd", "relu_sum3", 16, 3))

# --- cat_pipe_kernel: long segments at every lane mapping (q = d / 4 float4 per row), the gin aggregation, per-node b, self blocks, block caps
for _q, _k in ((2, CP(8, 1, 4)), (8, CP(8, 1, 4)), (9, CP(16, 1, 4)), (16, CP(16, 1, 4)), (17, CP(32, 1, 4)), (32, CP(32, 1, 4)), (33, CP(64, 1, 4)),
               (75, CP(64, 2, 4)), (150, CP(64, 4, 2)), (256, CP(64, 4, 2))):
    K("catpipe_long_q%d" % _q, CAT, (0, 4 * _q, 0), [_k], n=520)
K("catpipe_gin_d68", CAT, (68, 0, 0), [CP(32, 1, 2)], [N_GEN], profile="sparse", grads="a")
K("catpipe_gin_d128", CAT, (128, 0, 0), [CP(32, 1, 2)], profile="sparse")
K("catpipe_b_per_node", CAT, (8, 24, 0), [CP(8, 1, 4)], [N_GEN], bpn=True, grads="ab")
K("catpipe_self1", CAT, (0, 300, 0), [CP(64, 2, 4, ext=1)], [E_CAT4, S_FLAT], selfs=(("n", 300),), eps=0.5, grads="bse")
K("catpipe_self2", CAT, (0, 300, 0), [CP(64, 2, 4, ext=1)], [E_CAT4, S_GEN], selfs=(("n", 100), ("1", 200)), eps=0.25, grads="bse")
K("catpipe_self3", CAT, (100, 200, 0), [CP(64, 2, 4, ext=1)], [E_CAT4, N_GEN, S_GEN], selfs=(("1", 4), ("n", 200), ("n", 96)), eps=0.5, grads="abse")
for _b in (1, 2):
    K("catpipe_cap%d_32lanes" % _b, CAT, (64, 40, 8), [CP(32, 1, 4)], env=("GSN_PROP_CP", "32,4,%d" % _b), steady=("fwd", "cat_pipe", 8, 3))
    K("catpipe_cap%d_64lanes" % _b, CAT, (100, 200, 0), [CP(64, 2, 4)], env=("GSN_PROP_CP", "64,4,%d" % _b), steady=("fwd", "cat_pipe", 4, 3))
K("catpipe_cap1_self", CAT, (100, 200, 0), [CP(64, 2, 4, ext=1)], selfs=(("n", 296), ("1", 4)), eps=0.25, env=("GSN_PROP_CP", "64,4,1"),
  steady=("fwd", "cat_pipe", 4, 3))

# --- propagate_fwd_kernel<4, ..>: the aligned ladder (relu-sum outside 132 .. 384, relu-sum with per-node b, concatenations with the pipeline off)
K("fwd4_8_1_relu_d4", RELU, (4, 4, 4), [F(4, 8, 1)], [E_R4P, N_E4P], grads="abc")
K("fwd4_8_1_relu_d4_fold", RELU, (4, 4, 4), [F(4, 8, 1, ext=1, u4=0)], [E_R4P, N_FOLD], selfs=("a",), eps=0.5, grads="abce")
K("fwd4_16_1_relu_d64", RELU, (64, 64, 64), [F(4, 16, 1)], profile="sparse")
K("fwd4_16_1_relu_d64_ext", RELU, (64, 64, 0), [F(4, 16, 1, ext=1, u4=0)], [E_R4P, N_E4P, S_GEN], profile="sparse", selfs=(("n", 64), ("1", 64)), eps=0.25,
  grads="abse")
K("fwd4_16_1_plain", RELU, (64, 64, 64), [F(4, 16, 1, u4=0)], n=2100, profile="sparse")
K("fwd4_16_2_relu_d128_short", RELU, (128, 128, 128), [F(4, 16, 2)], profile="sparse")
K("fwd4_32_1_relu_d128_long", RELU, (128, 128, 128), [F(4, 32, 1)])
K("fwd4_64_1_relu_d256_b_per_node", RELU, (256, 256, 0), [F(4, 64, 1)], bpn=True, profile="sparse")         # (132 .. 384 per edge: relu_sum3)
K("fwd4_64_1_plain", RELU, (256, 256, 0), [F(4, 64, 1, u4=0)], n=520, bpn=True, profile="sparse")
K("fwd4_32_3_relu_b_per_node", RELU, (300, 300, 300), [F(4, 32, 3)], [E_R4P, N_E4P], bpn=True, grads="abc")
K("fwd4_32_3_cat_pipe_off", CAT, (0, 300, 0), [F(4, 32, 3)], n=520, env=("GSN_PROP_CP", "0"))
K("fwd4_64_2_relu_d512", RELU, (512, 512, 0), [F(4, 64, 2)], profile="sparse")
K("fwd4_64_4_relu_d1024", RELU, (1024, 1024, 0), [F(4, 64, 4)], [E_R4, N_E4], grads="ab")
K("fwd4_16_2_cat_pipe_off_ext", CAT, (64, 40, 8), [F(4, 16, 2, ext=1, u4=0)], profile="sparse", selfs=(("n", 112),), env=("GSN_PROP_CP", "0"))
# one case per rows-per-wave class beyond the 8 192-workgroup cap: the target loop strides
K("fwd4_stride_lpr16", RELU, (36, 0, 0), [F(4, 16, 1, u4=0)], n=131100, profile="sparse", grids={"propagate_fwd": 8192})
K("fwd4_stride_lpr32", RELU, (68, 0, 0), [F(4, 32, 1, u4=0)], n=65600, grids={"propagate_fwd": 8192})
K("fwd4_stride_lpr64", RELU, (132, 0, 0), [F(4, 64, 1, u4=0)], n=33001, profile="sparse", grids={"propagate_fwd": 8192})

# --- propagate_fwd_kernel<1, ..>: widths that are no multiple of four, zero columns, self blocks; the generic adjoints
K("fwd1_w3", CAT, (3, 0, 0), [F(1, 16, 1)], [N_GEN], profile="sparse", grads="a")
K("fwd1_w30", CAT, (10, 20, 0), [F(1, 32, 1)], [E_GEN, N_GEN], profile="sparse", grads="ab")
K("fwd1_w50", CAT, (20, 30, 0), [F(1, 64, 1)], profile="sparse")
K("fwd1_w130", CAT, (0, 130, 0), [F(1, 64, 4)], profile="sparse")
K("fwd1_w255", CAT, (100, 100, 55), [F(1, 64, 4)], [E_GEN, N_GEN], grads="abc")
K("fwd1_w301", CAT, (0, 301, 0), [F(1, 64, 16)])
K("fwd1_w1023", CAT, (1000, 0, 23), [F(1, 64, 16)], n=37)
K("fwd1_pads_1_1", CAT, (8, 8, 8), [F(1, 32, 1, ext=1, u4=0)], [E_GEN, N_GEN], pads=(1, 1), grads="abc")
K("fwd1_pads_1_0", CAT, (4, 4, 0), [F(1, 16, 1, ext=1, u4=0)], [E_GEN, N_GEN], pads=(1, 0), grads="ab", profile="sparse")
K("fwd1_pads_0_3", CAT, (4, 4, 4), [F(1, 16, 1, ext=1, u4=0)], [E_GEN], pads=(0, 3), grads="bc")
K("fwd1_self2", CAT, (0, 50, 0), [F(1, 64, 1, ext=1, u4=0)], [E_GEN, S_GEN], selfs=(("n", 20), ("1", 30)), eps=0.5, grads="bse", profile="sparse")
K("fwd1_self1_row", CAT, (0, 50, 0), [F(1, 64, 1, ext=1, u4=0)], [S_GEN], selfs=(("1", 50),), eps=0.25, grads="se", n=37)
K("fwd1_relu_d33", RELU, (33, 33, 33), [F(1, 64, 1)], [E_GEN, N_GEN], grads="abc")

# --- the remaining variants of every rung the default dispatch reaches: EXT (self term or zero columns), U4 (at most 128 workgroups) and plain
K("rs3_d384_ab_self", RELU, (384, 384, 0), [RS(32, 3, 2, ext=1, c=0)], [E_R4, N_E4], selfs=(("n", 384),), eps=0.25, grads="ab")
for _w, _k in ((32, CP(8, 1, 4, ext=1)), (64, CP(16, 1, 4, ext=1)), (128, CP(32, 1, 4, ext=1)), (132, CP(64, 1, 4, ext=1)), (600, CP(64, 4, 2, ext=1))):
    K("catpipe_long_d%d_self" % _w, CAT, (0, _w, 0), [_k], selfs=(("n", _w - 4), ("1", 4)), eps=0.5)
K("catpipe_gin_d68_self", CAT, (68, 0, 0), [CP(32, 1, 2, ext=1)], profile="sparse", selfs=(("1", 8), ("n", 60)), eps=0.25)
K("fwd4_32_1_ext", RELU, (128, 128, 128), [F(4, 32, 1, ext=1, u4=0)], selfs=(("n", 128),), eps=0.5)
K("fwd4_64_1_ext", RELU, (256, 256, 0), [F(4, 64, 1, ext=1, u4=0)], bpn=True, profile="sparse", selfs=("a",), eps=0.25)
K("fwd4_32_3_ext", RELU, (300, 300, 300), [F(4, 32, 3, ext=1, u4=0)], bpn=True, selfs=(("n", 300), ("1", 300)), eps=0.5)
K("fwd4_64_2_ext", RELU, (512, 512, 0), [F(4, 64, 2, ext=1, u4=0)], profile="sparse", selfs=(("n", 512),), eps=0.25)
K("fwd4_64_4_ext", CAT, (512, 256, 256), [F(4, 64, 4, ext=1, u4=0)], profile="sparse", selfs=(("n", 500), ("1", 24), ("n", 500)), eps=0.5)
K("fwd4_16_2_plain", RELU, (128, 128, 128), [F(4, 16, 2, u4=0)], n=2100, profile="sparse")
K("fwd4_32_3_plain", RELU, (300, 300, 0), [F(4, 32, 3, u4=0)], n=1100, bpn=True, profile="sparse")
K("fwd4_64_2_plain", RELU, (512, 512, 0), [F(4, 64, 2, u4=0)], n=520, profile="sparse")
K("fwd4_64_4_plain", RELU, (1024, 1024, 0), [F(4, 64, 4, u4=0)], n=520, profile="sparse")
K("fwd1_16_1_plain", CAT, (3, 0, 0), [F(1, 16, 1, u4=0)], n=2100, profile="sparse")
K("fwd1_64_1_plain", CAT, (20, 30, 0), [F(1, 64, 1, u4=0)], n=520, profile="sparse")
K("fwd1_64_4_plain", CAT, (0, 130, 0), [F(1, 64, 4, u4=0)], n=520, profile="sparse")
K("fwd1_64_16_plain", CAT, (0, 301, 0), [F(1, 64, 16, u4=0)], n=520, profile="sparse")
# several column chunks per lane with zero columns and self blocks: the offsets of pads and blocks cross chunk boundaries
K("fwd1_64_4_pads", CAT, (100, 100, 50), [F(1, 64, 4, ext=1, u4=0)], [E_GEN, N_GEN], pads=(1, 1), grads="abc")
K("fwd1_64_4_pads_self", CAT, (63, 66, 61), [F(1, 64, 4, ext=1, u4=0)], [E_GEN, N_GEN, S_GEN], pads=(2, 3), selfs=(("n", 65), ("1", 64), ("n", 66)), eps=0.5,
  grads="abcse")
K("fwd1_64_16_self", CAT, (0, 301, 0), [F(1, 64, 16, ext=1, u4=0)], [E_GEN, S_GEN], selfs=(("n", 150), ("1", 151)), eps=0.25, grads="bse")
K("fwd1_64_16_pad", CAT, (1000, 0, 23), [F(1, 64, 16, ext=1, u4=0)], [E_GEN, N_GEN], n=37, pads=(0, 1), grads="ac")
K("fwd1_64_16_pads_self", CAT, (300, 301, 302), [F(1, 64, 16, ext=1, u4=0)], pads=(3, 1), selfs=(("1", 5), ("n", 900), ("n", 2)), eps=0.5)
# widths that are multiples of four behind pointers that are not 16-byte aligned (a storage offset of one float): the scalar kernels forward;
# backward the gradients are fresh, aligned tensors, so only the passes that read the forward inputs (the relu mask, the self block) go scalar
K("misaligned_cat", CAT, (8, 24, 0), [F(1, 32, 1)], [E_CAT4, N_GEN], profile="sparse", grads="ab", offset=1)
K("misaligned_relu_d300", RELU, (300, 300, 300), [F(1, 64, 16)], [E_GEN, N_E4P], grads="abc", offset=1)
K("misaligned_self", CAT, (0, 16, 0), [F(1, 16, 1, ext=1, u4=0)], [E_CAT4, S_GEN], selfs=(("n", 16),), eps=0.5, grads="bse", offset=1)

# --- no edges at all: the self term alone, or zeros
K("edgeless_self", CAT, (0, 16, 0), [F(4, 8, 1, ext=1, u4=0)], [S_FLAT], n=37, profile="empty", selfs=(("n", 16),), eps=0.5, grads="se")
K("edgeless_zero", CAT, (0, 16, 0), [F(4, 8, 1)], n=37, profile="empty")
K("edgeless_relu_self", RELU, (5, 5, 0), [F(1, 16, 1, ext=1, u4=0)], n=37, profile="empty", selfs=(("n", 5),), eps=0.25)

# --- the adjoints
K("bwd_cat4_b", CAT, (0, 16, 0), [WG], [E_CAT4], grads="b")
K("bwd_cat4_300", CAT, (0, 300, 0), [WG], [E_CAT4], grads="b")
K("bwd_cat4_b_only", CAT, (64, 40, 8), [CP(32, 1, 4)], [E_CAT4], grads="b")
K("bwd_cat4_c_only", CAT, (64, 40, 8), [CP(32, 1, 4)], [E_CAT4], grads="c")
K("bwd_cat4_abc", CAT, (64, 40, 8), [CP(32, 1, 4)], [E_CAT4, N_GEN], grads="abc")
K("bwd_relu4p_b_only", RELU, (320, 320, 320), [RS(16, 5, 2)], [E_R4P], grads="b")
K("bwd_relu4p_c_only", RELU, (300, 300, 300), [RS(16, 5, 2)], [E_R4P, N_E4P], grads="ac")
K("bwd_fold_d132", RELU, (132, 132, 0), [RS(16, 5, 1, ext=1, c=0)], [E_R4P, N_FOLD], selfs=("a",), eps=0.25, grads="abe", profile="sparse")
K("bwd_fold_d320", RELU, (320, 0, 320), [RS(16, 5, 1, ext=1, c=0)], [E_R4P, N_FOLD], selfs=("a",), eps=0.5, grads="ace")
K("bwd_node_relu_only_a", RELU, (300, 300, 300), [RS(16, 5, 2)], [N_GEN], grads="a")
K("bwd_node_relu_b_per_node_no_c", RELU, (64, 64, 0), [F(4, 16, 1)], [N_GEN], bpn=True, grads="ab", profile="sparse")
K("bwd_self_rows_stride", CAT, (0, 68, 0), [F(4, 16, 2, ext=1, u4=0)], [E_CAT4, S_GEN], n=5000, profile="sparse", selfs=(("1", 4), ("n", 64)), eps=0.5,
  grads="bse", grids={"propagate_self_bwd": 1024})
# beyond the grid caps of the adjoints (16 384 workgroups: 16 edges or vertices each, 4 vertices or 256 elements in the generic kernels)
K("big_generic_edge_and_node", CAT, (10, 20, 0), [F(1, 32, 1, u4=0)], [E_GEN, N_GEN], n=100001, profile="sparse", grads="ab",
  grids={"propagate_fwd": 8192, "propagate_bwd_edge": 16384, "propagate_bwd_node": 16384})
K("big_cat4", CAT, (0, 4, 4), [F(4, 8, 1, u4=0)], [E_CAT4], n=792145, profile="sparse", grads="bc", grids={"propagate_fwd": 8192, "propagate_bwd_edge_cat4": 16384})
K("big_relu4p", RELU, (8, 8, 0), [F(4, 8, 1, u4=0)], [E_R4P, N_E4P], n=792145, profile="sparse", grads="ab",
  grids={"propagate_fwd": 8192, "propagate_bwd_edge_relu4p": 16384, "propagate_bwd_node_edge4p<fold0>": 16384}, steady=("bwd", "propagate_bwd_node_edge4p", 16, 3))
K("big_fold", RELU, (8, 8, 0), [F(4, 8, 1, ext=1, u4=0)], [E_R4P, N_FOLD], n=792145, profile="sparse", selfs=("a",), eps=0.25, grads="abe",
  grids={"propagate_bwd_edge_relu4p": 16384, "propagate_bwd_node_edge4p<fold1>": 16384}, steady=("bwd", "propagate_bwd_node_edge4p", 16, 3))
K("big_self_flat", RELU, (16, 0, 0), [F(4, 8, 1, ext=1, u4=0)], [N_GEN, S_FLAT], n=300000, profile="sparse", selfs=("a",), eps=0.5, grads="ae",
  grids={"propagate_fwd": 8192, "propagate_bwd_node": 16384, "propagate_self_bwd_flat": 4096})

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------
# one case: the call, its fp64 reference, the routes
# ------------------------------------------------------------------------------------------------------------------
class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        if self.env:
            self.old = os.environ.get(self.env[0])
            os.environ[self.env[0]] = self.env[1]

    def __exit__(self, *exc):
        if self.env:
            if self.old is None:
                del os.environ[self.env[0]]
            else:
                os.environ[self.env[0]] = self.old
        return False


def _reference(case, ei, n, t):
    """fp64, plain torch: t holds the leaves a, b, c, eps, s0 .. s2 (or None)."""
    src, tgt = ei[0], ei[1]
    E = src.numel()
    a, b, c = t["a"], t["b"], t["c"]
    if case["kind"] == CAT:
        zeros = lambda w: torch.zeros(E, w, dtype=torch.float64, device=DEV)
        parts = [] if a is None else [a[src]]
        if b is not None:
            parts += [zeros(case["pads"][0]), b[src] if case["bpn"] else b]
        if c is not None:
            parts += [zeros(case["pads"][1]), c]
        msg = torch.cat(parts, 1)
    else:
        pre = 0
        if a is not None:
            pre = pre + a[src]
        if b is not None:
            pre = pre + (b[src] if case["bpn"] else b)
        if c is not None:
            pre = pre + c
        msg = torch.where(pre > 0, pre, torch.zeros_like(pre))          # the kernels' convention: a pre-activation of exactly zero passes nothing
        t["zero_share"] = float((pre.detach() == 0).double().mean()) if E else 0.0
    out = torch.zeros(n, msg.shape[1], dtype=torch.float64, device=DEV).index_add(0, tgt, msg)
    blocks = [t[k].expand(n, -1) for k in ("s0", "s1", "s2") if t.get(k) is not None]
    if blocks:
        own = torch.cat(blocks, 1) if case["kind"] == CAT else sum(blocks)
        out = out + (1 + (t["eps"] if t["eps"] is not None else 0)) * own
    return out


def _offset_view(t, offset):
    """the same values as a contiguous view that starts ``offset`` floats into its storage (data_ptr() % 16 = 4 * offset)."""
    if not offset:
        return t
    store = torch.empty(t.numel() + offset, dtype=t.dtype, device=t.device)
    view = store[offset:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
    return view


def _differences(what, got, want64):
    want = want64.to(torch.float32)
    if got.shape == want.shape and torch.equal(got, want):
        return []
    if got.shape != want.shape:
        return ["%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(want.shape))]
    bad = (got != want).reshape(got.shape[0], -1) if got.dim() > 1 else (got != want).reshape(-1, 1)
    rows = bad.any(1).nonzero().flatten()
    return ["%s: %d elements in %d rows differ (first rows %s)" % (what, int(bad.sum()), rows.numel(), rows[:8].tolist())]


def run_case(case):
    """dict(fwd, bwd: [(kernel, grid)] without the CSR builds; csr: the CSR kernels seen; bad: what differed; n, E, zero_share)."""
    from gsn_amd import _abi
    from gsn_amd import layers
    from gsn_amd._autograd import _segment_sum_cols
    n = case["n"]
    ei, _, _ = _graph(n, case["profile"])
    E = ei.shape[1]
    gen = torch.Generator(DEV).manual_seed(len(case["name"]) + 7 * n)
    real = _abi.lib()
    rec = _Routes(real)
    res = dict(n=n, E=E, bad=[], bwd=[], csr=[])

    def split(entries):
        res["csr"] += [k for k, _ in entries if k in CSR_KERNELS]
        return [(k, g) for k, g in entries if k not in CSR_KERNELS]

    if case["call"] == "segsum":
        rows64 = _dyadic(E, case["ld"], gen, nonzero=True)
        rows = rows64.to(torch.float32)
        _abi._lib = rec
        try:
            out = _segment_sum_cols(ei, 1, n, rows, case["col0"], case["width"])
            torch.cuda.synchronize()
        finally:
            _abi._lib = real
        res["fwd"] = split(rec.take())
        ref = torch.zeros(n, case["width"], dtype=torch.float64, device=DEV).index_add(0, ei[1], rows64[:, case["col0"]:case["col0"] + case["width"]])
        res["bad"] += _differences("out", out, ref)
        return res

    da, db, dc = case["widths"]
    nz = case["kind"] == CAT
    t = dict(a=_dyadic(n, da, gen, nz) if da else None, b=_dyadic(n if case["bpn"] else E, db, gen, nz) if db else None,
             c=_dyadic(E, dc, gen, nz) if dc else None, eps=None, s0=None, s1=None, s2=None)
    if case["eps"] is not None:
        t["eps"] = torch.tensor([case["eps"]], dtype=torch.float64, device=DEV)
    for k, spec in enumerate(case["selfs"]):
        t["s%d" % k] = t["a"] if spec == "a" else _dyadic(n if spec[0] == "n" else 1, spec[1], gen)
    wants = dict(a="a" in case["grads"], b="b" in case["grads"], c="c" in case["grads"], eps="e" in case["grads"])
    for k, spec in enumerate(case["selfs"]):
        wants["s%d" % k] = wants["a"] if spec == "a" else "s" in case["grads"]
    l64, l32 = {}, {}
    for k, v in t.items():
        if v is None:
            l64[k] = l32[k] = None
        elif k.startswith("s") and case["selfs"][int(k[1])] == "a":
            l64[k], l32[k] = l64["a"], l32["a"]                    # the same leaf: its two gradients are summed by autograd
        else:
            l64[k] = v.clone().requires_grad_(wants[k])
            l32[k] = _offset_view(v.to(torch.float32), case["offset"] if k != "eps" else 0).requires_grad_(wants[k])
    ref = _reference(case, ei, n, l64)
    res["zero_share"] = l64.pop("zero_share", None)
    selfs32 = tuple(l32["s%d" % k] for k in range(len(case["selfs"])))
    up64 = _dyadic(n, ref.shape[1], gen)
    _abi._lib = rec
    try:
        with _Env(case["env"]):
            out = layers.propagate(case["kind"], ei, 1, n, a=l32["a"], b=l32["b"], c=l32["c"], b_per_node=case["bpn"], selfs=selfs32, eps=l32["eps"],
                                   pads=case["pads"])
            torch.cuda.synchronize()
            res["fwd"] = split(rec.take())
            res["bad"] += _differences("out", out.detach(), ref.detach())
            if case["grads"]:
                (ref * up64).sum().backward()
                (out * up64.to(torch.float32)).sum().backward()
                torch.cuda.synchronize()
                res["bwd"] = split(rec.take())
    finally:
        _abi._lib = real
    seen = set()
    for k in l64:
        if l64[k] is not None and wants.get(k) and id(l64[k]) not in seen:
            seen.add(id(l64[k]))
            if l32[k].grad is None:
                res["bad"].append("g_%s: no gradient" % k)
            else:
                res["bad"] += _differences("g_" + k, l32[k].grad, l64[k].grad)
    return res


@functools.lru_cache(maxsize=None)
def result_of(name):
    return run_case(BY_NAME[name])


# ------------------------------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_matches_fp64_and_takes_its_route(case):
    res = result_of(case["name"])
    print(case["name"], "n=%d E=%d" % (res["n"], res["E"]), "fwd", res["fwd"], "bwd", res["bwd"], "bad", res["bad"], "zero", res.get("zero_share"))
    assert [k for k, _ in res["fwd"]] == case["fwd"]
    assert [k for k, _ in res["bwd"]] == case["bwd"]
    for kernel, grid in case["grids"].items():
        hits = [g for k, g in res["fwd"] + res["bwd"] if k == kernel or k.startswith(kernel + "<")]
        assert hits and all(g == grid for g in hits), (kernel, grid, hits)
    assert res["bad"] == []


def test_profiles_hold_the_degree_spread():
    for n, profile in ((37, "spread"), (203, "spread"), (203, "sparse"), (520, "spread"), (5000, "sparse")):
        ei, indeg, outdeg = _graph(n, profile)
        E = ei.shape[1]
        for deg in (indeg, outdeg):
            assert set(SPREAD) <= set(deg.tolist()), (n, profile)
            assert deg.max() == (E - deg.max()) // 2 or deg.max() == 2048               # the hub: a third of the edges
            assert deg.max() < (1 << 17)
        assert (E >= 8 * n) == (profile == "spread")
        assert bool((ei[1][1:] < ei[1][:-1]).any())                                          # edge order is not the target order
    assert _graph(37, "empty")[0].shape[1] == 0 and _graph(1, "spread")[0].shape[1] == 29


def test_relu_cases_hold_exact_zero_pre_activations():
    share = result_of("rs3_d300_abc_fold")["zero_share"]
    assert 0.02 < share < 0.07, share


def test_capped_cases_really_iterate():
    """Every case marked steady: n >= 3 * grid * rows per workgroup and a partial step behind the full ones (three steps consume every
    rotated register of the three-deep pipelines; the adjoints' cap of 16 384 workgroups is fixed, so their cases have 3 * 2^18 + 5 713 vertices)."""
    marked = [c for c in CASES if c["steady"]]
    assert len(marked) >= 12
    for case in marked:
        phase, kernel, per_wg, steps = case["steady"]
        res = result_of(case["name"])
        grids = [g for k, g in res[phase] if k.startswith(kernel)]
        assert len(grids) == 1, (case["name"], res[phase])
        step = grids[0] * per_wg
        if phase == "fwd":
            assert int(case["env"][1].split(",")[-1]) == grids[0], case["name"]
        assert steps >= 3 and case["n"] >= steps * step and case["n"] % step != 0, (case["name"], step)
        if phase == "bwd":                                     # the edge pass of the same case: the prefetch of the next edge's indices
            eg = [g for k, g in res["bwd"] if k == E_R4P]
            assert eg and res["E"] > 2 * eg[0] * 16 and res["E"] % (eg[0] * 16) != 0, (case["name"], res["E"])


EVERY_KERNEL = {
    WG,
    RS(16, 5, 1), RS(16, 5, 1, nt=1), RS(16, 5, 2), RS(16, 5, 2, nt=1), RS(16, 5, 2, c=0), RS(16, 5, 1, ext=1), RS(16, 5, 1, ext=1, c=0),
    RS(32, 3, 1), RS(32, 3, 1, nt=1), RS(32, 3, 2), RS(32, 3, 2, nt=1), RS(32, 3, 4), RS(32, 3, 4, nt=1), RS(32, 3, 4, c=0), RS(32, 3, 2, ext=1),
    RS(32, 3, 2, ext=1, c=0),
    RS(64, 2, 1), RS(64, 2, 1, nt=1), RS(64, 2, 2), RS(64, 2, 2, nt=1), RS(64, 2, 4), RS(64, 2, 4, nt=1),
    # cat_pipe: the seven mappings the default rule picks, without and with self blocks
    CP(8, 1, 4), CP(16, 1, 4), CP(32, 1, 4), CP(32, 1, 2), CP(64, 1, 4), CP(64, 2, 4), CP(64, 4, 2),
    CP(8, 1, 4, ext=1), CP(16, 1, 4, ext=1), CP(32, 1, 4, ext=1), CP(32, 1, 2, ext=1), CP(64, 1, 4, ext=1), CP(64, 2, 4, ext=1), CP(64, 4, 2, ext=1),
    # propagate_fwd: every rung of the aligned and of the scalar ladder as U4 (grid <= 128), plain and EXT
    *[F(v, l, m, ext=e, u4=u) for v, l, m in ((4, 8, 1), (4, 16, 1), (4, 16, 2), (4, 32, 1), (4, 64, 1), (4, 32, 3), (4, 64, 2), (4, 64, 4),
                                             (1, 16, 1), (1, 32, 1), (1, 64, 1), (1, 64, 4), (1, 64, 16)) for e, u in ((0, 1), (0, 0), (1, 0))],
    E_GEN, E_CAT4, E_R4, E_R4P, N_GEN, N_E4, N_E4P, N_FOLD, S_FLAT, S_GEN,
}


def test_table_reaches_every_kernel():
    """The kernels the table reports, template arguments included, are exactly this list: a rung added without a case, or a threshold that
    moves a case to another kernel, fails here.  The list is every instantiation the dispatch rules reach without a forcing variable:
    13 rungs of propagate_fwd x (U4, plain, EXT), 7 cat_pipe mappings x (plain, EXT), relu_sum3 at 16 and 32 lanes x (two, three streams) x
    (plain, EXT), the adjoints.  On top of it the relu_sum3 mappings GSN_PROP_RS forces (three streams, no self term).  Left out: what only
    GSN_PROP_LPR (read once per process) or a forced GSN_PROP_CP mapping reaches -- test_forced_mappings_keep_the_bits runs some of the
    latter against the unforced bits -- and edge_split_sum, csr_graphs and segsum_prepare, which have their own tests."""
    seen, csr = set(), set()
    for case in CASES:
        res = result_of(case["name"])
        seen |= {k for k, _ in res["fwd"] + res["bwd"]}
        csr |= set(res["csr"])
    assert seen == EVERY_KERNEL, (sorted(seen - EVERY_KERNEL), sorted(EVERY_KERNEL - seen))
    assert csr == CSR_KERNELS, sorted(CSR_KERNELS - csr)          # (the table's own index builds: one workgroup below 12 288 vertices, seven launches above)


def _forced(kind, widths, selfs, eps, envs, var):
    from gsn_amd import _abi, layers
    n = 203
    ei, _, _ = _graph(n, "spread")
    E = ei.shape[1]
    gen = torch.Generator(DEV).manual_seed(11)
    da, db, dc = widths
    a, b, c = [_dyadic(r, w, gen, kind == CAT).float() if w else None for r, w in ((n, da), (E, db), (E, dc))]
    own = tuple(a if s == "a" else _dyadic(n if s[0] == "n" else 1, s[1], gen).float() for s in selfs)
    e = None if eps is None else torch.tensor([eps], device=DEV)
    base = layers.propagate(kind, ei, 1, n, a=a, b=b, c=c, selfs=own, eps=e)
    for env in envs:
        with _Env((var, env)):
            got = layers.propagate(kind, ei, 1, n, a=a, b=b, c=c, selfs=own, eps=e)
            route = _abi.lib().gsn_propagate_last_route().decode()
        assert torch.equal(got, base), (env, route)
        yield env, route


def test_forced_mappings_keep_the_bits():
    """One relu-sum and one concatenation shape: every forced mapping and every block cap gives the unforced call's bits."""
    rs = ["0"] + ["%d,%d,%d" % (l, u, nt) for l in (16, 32, 64) for u in (1, 2, 4) if not (l == 16 and u == 4) for nt in (0, 1)]
    rs += ["16,0,0,1", "16,0,0,2", "16,0,0,5", "32,0,0,1", "32,4,1,2", "64,2,0,1", "64,4,0,3"]
    for selfs, eps in (((), None), (("a",), 0.25)):
        routes = dict(_forced(RELU, (300, 300, 300), selfs, eps, rs, "GSN_PROP_RS"))
        assert routes["0"].startswith("propagate_fwd<4,32,3") and all(r.startswith("relu_sum3<") for k, r in routes.items() if k != "0")
        assert routes["16,0,0,5"].endswith("grid=5") and routes["64,4,0,3"].endswith("grid=3")
    cp = ["0", "64,4", "64,2", "64,1", "32,2", "32,1", "16,2", "16,1", "64,4,1", "64,4,2", "64,2,3", "32,2,1", "16,2,2"]
    for selfs, eps in (((), None), ((("n", 100), ("1", 200)), 0.5)):
        routes = dict(_forced(CAT, (100, 200, 0), selfs, eps, cp, "GSN_PROP_CP"))
        assert routes["0"].startswith("propagate_fwd<4,32,3") and all(r.startswith("cat_pipe<") for k, r in routes.items() if k != "0")
        assert routes["32,2"].startswith("cat_pipe<32,3,2") and routes["16,1"].startswith("cat_pipe<16,5,1") and routes["64,2,3"].endswith("grid=3")


# ------------------------------------------------------------------------------------------------------------------
# CSR build: the one-workgroup kernel's limits and the scan tiles of the multi-launch build
# ------------------------------------------------------------------------------------------------------------------
SMALL = ["csr_small"]
MULTI = ["csr_zero", "csr_hist", "scan_tile_sums", "scan_tile_offsets", "scan_apply", "csr_fill", "csr_sort_segments"]
SCAN_TILE = 1024
CSR_POINTS = [(12287, 32768, SMALL), (12288, 32768, MULTI), (12287, 32769, MULTI), (12288, 0, ["csr_zero", "scan_tile_sums", "scan_tile_offsets", "scan_apply"]),
              (7, 0, SMALL)]
# n + 1 counters around one scan tile, around two (the first count that needs a second tile is SCAN_TILE + 1) and around the 64 tile sums one
# pass of scan_tile_offsets takes; the same counts in the one-workgroup kernel, whose scan passes are 1 024 wide as well
CSR_POINTS += [(k * SCAN_TILE + o - 1, 40000, MULTI) for k in (1, 2, 64) for o in (-1, 0, 1)]
CSR_POINTS += [(k * SCAN_TILE + o - 1, 5000, SMALL) for k in (1, 2) for o in (-1, 0, 1)]


@pytest.mark.parametrize("n,E,route", CSR_POINTS, ids=["n%d_E%d" % (n, E) for n, E, _ in CSR_POINTS])
def test_csr_build_boundaries(n, E, route):
    """seg_ptr, perm, sorted_target and sorted_other against a stable sort and bincount; one hub, several empty vertices (the last one among them)."""
    from gsn_amd import _abi
    from gsn_amd._index import build_csr
    rng = np.random.default_rng(n + E)
    alive = rng.permutation(n - 1)[:max(1, (n * 3) // 4)]             # a quarter of the vertices and the last one own no edge
    index = alive[rng.integers(0, alive.size, E)]
    index[rng.permutation(E)[:min(E // 3, 2000)]] = alive[0]          # the hub
    index = torch.from_numpy(index.astype(np.int64)).to(DEV)
    other = torch.from_numpy(rng.integers(0, n, E).astype(np.int64)).to(DEV)
    seg_ptr, perm, tgt, src = build_csr(index, n, with_targets=True, other=other)
    got = [k for k, _ in map(_parse, [x for x in _abi.lib().gsn_propagate_last_route().decode().split(";") if x])]
    torch.cuda.synchronize()
    assert got == route
    counts = torch.bincount(index, minlength=n)
    want_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), counts.cumsum(0)])
    assert torch.equal(seg_ptr.long(), want_ptr)
    if E:
        assert int(counts.max()) >= min(E // 3, 2000) and int((counts == 0).sum()) >= n // 4 - 1 and int(counts[-1]) == 0
    values, order = torch.sort(index, stable=True)
    assert torch.equal(perm.long(), order) and torch.equal(tgt.long(), values) and torch.equal(src.long(), other[order])
