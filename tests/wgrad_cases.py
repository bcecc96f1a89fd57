"""The case table of tests/test_wgrad_bf16_gpu.py and tests/wgrad_child.py (not a test module): every weight-gradient call gsn_wgrad_hip is
tested on, gW += gH^T [X_0 | ... | X_4], built on the CPU from a seeded generator, so that the test process and its child processes hold the same
tensors bit for bit.

A block of X is `plain` (row m of the block is row m of its tensor) or gathered through a row index (`g32`: int32, `g64`: int64; row m is
table[idx[m]], the x_i / x_j blocks of an edge stage).  Everything around the rows a call may read is poisoned with NaN, at valid addresses, so that
a wrong read shows as a NaN in gW and not as a fault:
  * gH and the plain blocks carry 64 NaN rows behind row m_rows;
  * every table row r with r % 7 == 3 is NaN and no index names it;
  * every index array carries 64 entries behind m_rows, all pointing at NaN row 3;
  * gW is a view into a buffer with 4 096 sentinel floats on each side (gw_buffer).
Magnitudes are those of test_eval_grad_gpu.py::test_weight_gradient_bf16x6_vs_fp64: gH = randn * logspace(-6, 6, n_out), blocks randn * logspace(-3, 3, width)."""
import collections
import re
import zlib

import torch

PAD_ROWS = 64            # NaN rows behind gH / a plain block, entries behind an index array
GUARD = 4096             # sentinel floats on each side of gW
SENTINEL = -24680.125
NAN_ROW = 3              # table rows r % 7 == NAN_ROW are NaN

Spec = collections.namedtuple("Spec", "m_rows n_out blocks slabs default_only shared")
# slabs: (slabs, rows per slab) the case is there for under default switches -- what the trace line must report
# shared: gathered blocks of equal width and table size read ONE table (x_i and x_j of an edge stage)


def _specs():
    t = collections.OrderedDict()
    lists = {"one": [(7, "plain", None)], "two": [(4, "plain", None), (3, "plain", None)], "mixed": [(3, "g64", 5), (1, "plain", None), (3, "g32", 200)]}
    # row ladder, one slab: the pipeline's fill and drain states (16 rows per step, two register sets that take turns)
    for m in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64):
        for tag, blocks in lists.items():
            t["rows%d_%s" % (m, tag)] = Spec(m, 9, blocks, (1, 64), False, False)
    # slab edges: a last slab of one row; a ninth slab (the second group of eight of the workgroup map, seven workgroups leave at once)
    for m, slabs in ((65, (2, 64)), (513, (9, 64))):
        for tag, blocks in lists.items():
            t["rows%d_%s" % (m, tag)] = Spec(m, 9, blocks, slabs, False, False)
    # 2 x 2 tiles with ragged edges of 2 and 1 columns, a block seam at column 64 / 65, a block across the tile edge, last slab of 9 rows
    t["tiles_seams"] = Spec(777, 130, [(64, "g64", 50), (1, "plain", None), (64, "g32", 1000)], (13, 64), False, False)
    t["five_blocks"] = Spec(777, 70, [(33, "g32", 500), (5, "plain", None), (128, "g64", 2000), (3, "g64", 40), (4, "plain", None)], (13, 64), False, False)
    t["wide"] = Spec(3000, 257, [(36, "g64", 997)], (47, 64), False, False)
    t["middle"] = Spec(5000, 600, [(148, "g64", 1200), (152, "g32", 1200)], (16, 320), False, False)
    # the edge stage of the headline model's size, x_i and x_j on one table; the 2 048-workgroup cap (default switches only: the slab rule)
    t["edge_stage"] = Spec(100000, 128, [(128, "g64", 30000), (128, "g32", 30000), (4, "plain", None)], (196, 512), True, True)
    t["cap"] = Spec(70001, 600, [(300, "plain", None)], (137, 512), True, False)
    return t


SPECS = _specs()


def names(default_process=True):
    """case names; default_process=False leaves out the cases that are about the default slab rule"""
    return [n for n, s in SPECS.items() if default_process or not s.default_only]


Case = collections.namedtuple("Case", "name m_rows n_out blocks gh data idx")
# gh: [m_rows + 64, n_out]; data[b]: [m_rows + 64, width] (plain) or [table_rows, width] (gathered); idx[b]: None or [m_rows + 64] int32 / int64


def build(name):
    """The CPU tensors of one case (deterministic: the generator is seeded with the name)."""
    s = SPECS[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    m = s.m_rows

    def rows(n, width, lo, hi):
        return torch.randn(n, width, generator=g) * torch.logspace(lo, hi, width)

    gh = torch.cat([rows(m, s.n_out, -6, 6), torch.full((PAD_ROWS, s.n_out), float("nan"))])
    data, idx, tables = [], [], {}
    for width, kind, table_rows in s.blocks:
        if kind == "plain":
            data.append(torch.cat([rows(m, width, -3, 3), torch.full((PAD_ROWS, width), float("nan"))]))
            idx.append(None)
            continue
        assert table_rows > NAN_ROW
        key = (width, table_rows)
        if not (s.shared and key in tables):
            tab = rows(table_rows, width, -3, 3)
            tab[NAN_ROW::7] = float("nan")
            tables[key] = tab
        valid = torch.tensor([r for r in range(table_rows) if r % 7 != NAN_ROW])
        ix = valid[torch.randint(0, len(valid), (m,), generator=g)]              # unsorted, with repeats
        ix = torch.cat([ix, torch.full((PAD_ROWS,), NAN_ROW, dtype=torch.int64)])
        data.append(tables[key])
        idx.append(ix.to(torch.int32 if kind == "g32" else torch.int64))
    return Case(name, m, s.n_out, s.blocks, gh, data, idx)


def to_device(case, dev):
    return case._replace(gh=case.gh.to(dev), data=[t.to(dev) for t in case.data], idx=[None if i is None else i.to(dev) for i in case.idx])


def assembled(case):
    """The same case with every gathered block replaced by its materialised rows table[idx] (NaN rows behind m_rows included)."""
    data = [t if i is None else t[i.long()] for t, i in zip(case.data, case.idx)]
    return case._replace(data=data, idx=[None] * len(data), blocks=[(w, "plain", None) for w, _, _ in case.blocks])


def x_rows(case):
    """[m_rows, K]: the rows of X the call is given"""
    return torch.cat([(t if i is None else t[i.long()])[:case.m_rows] for t, i in zip(case.data, case.idx)], 1)


def k_total(case):
    return sum(w for w, _, _ in case.blocks)


def gw_buffer(case, dev, fill=None):
    """(buffer, view): gW as a [n_out, K] view into a buffer with GUARD sentinel floats on each side; zeros, or a copy of `fill`"""
    n = case.n_out * k_total(case)
    buf = torch.full((2 * GUARD + n,), SENTINEL, device=dev)
    view = buf[GUARD:GUARD + n].view(case.n_out, k_total(case))
    if fill is None:
        view.zero_()
    else:
        view.copy_(fill)
    return buf, view


def guards_intact(buf):
    s = torch.tensor(SENTINEL).view(torch.int32).item()
    b = buf.view(torch.int32)
    return bool((b[:GUARD] == s).all()) and bool((b[-GUARD:] == s).all())


def launch(case, gw):
    """gsn_wgrad_hip on the device tensors of `case`, into gw; the status is checked"""
    from gsn_amd import _abi
    arr = (_abi.gsn_block * len(case.data))()
    for b, (t, i) in enumerate(zip(case.data, case.idx)):
        arr[b].data = t.data_ptr(); arr[b].width = t.shape[1]
        arr[b].idx = i.data_ptr() if i is not None and i.dtype == torch.int64 else None
        arr[b].idx32 = i.data_ptr() if i is not None and i.dtype == torch.int32 else None
    _abi.check(_abi.lib().gsn_wgrad_hip(case.m_rows, case.n_out, case.gh.data_ptr(), len(case.data), arr, gw.data_ptr(), _abi.current_stream()), "gsn_wgrad_hip")


TRACE = re.compile(r"gsn wgrad: M (\d+) N (\d+) K (\d+) blocks (\d+)( gathered)? slabs (\d+) x (\d+) rows (\S+)$", re.M)
Route = collections.namedtuple("Route", "m_rows n_out k blocks gathered slabs slab_rows kernel")


def routes(text):
    """every weight-gradient line of a GSN_CHAIN_TRACE output, in order"""
    return [Route(int(a), int(b), int(c), int(d), bool(e), int(f), int(h), k) for a, b, c, d, e, f, h, k in TRACE.findall(text)]


def expected_kernel(n_blocks, gathered, pipe=6, fp32=False):
    """the kernel gsn_wgrad_hip launches for a block list under GSN_WGRAD_PIPE=pipe / GSN_WGRAD_FP32: gathered calls take the one depth-6 gather
    kernel at every depth but 0, and under the fp32 switch too"""
    if gathered:
        return "wgrad_bf16_pipe_kernel<gather,6>" if pipe else "wgrad_bf16_kernel<gather>"
    if fp32:
        return "wgrad_kernel"
    if not pipe:
        return "wgrad_bf16_kernel<plain>"
    return "wgrad_bf16_pipe_kernel<%s,%d>" % ("single" if n_blocks == 1 else "blocks", pipe)
