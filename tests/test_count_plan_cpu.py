"""The counting launch planner (gsn_amd/csrc/count_plan.cpp: count_plan) on the CPU, compiled for the host by the test-only harness
tests/count_plan_harness.cpp.  tests/golden/count_launch_plans.json holds launches recorded from the launcher before the planner was cut
out of it -- the request, how its plan table is built, the switch texts, and the answer: the refusal's status and full text, or W, T, kernel,
grid, LDS bytes, the status memset and every field of the argument block (pointer fields by the request pointer they equal).  Every case is
replayed and every recorded item must be equal."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "count_launch_plans.json")
KERNELS = ("GENERIC", "GENERIC_TAIL", "DIRECTED", "DIRECTED_TAIL", "MOL", "CYCLE_ANY", "CYCLE_KEYS")      # count_plan.h: enum CountKernel
ENC_MAX_COLS = 64
# every pointer a request can carry gets a made-up address of its own (never followed): slot i at (i + 1) << 36, plus the case's low bits
POINTERS = ("plan_dev", "node_ptr", "edge_ptr", "edge_index", "graph_ids", "out", "status", "enc_out", "enc16",
            "side.seg_ptr", "side.perm", "side.sorted_target", "side.sorted_other", "side.node_codes", "side.node_pack", "side.edge_codes",
            "side.code_status", "keys.nkey", "keys.ekeys", "keys.idmask")

with open(GOLDEN) as _f:
    _GOLDEN = json.load(_f)


def _expand(case):
    """A stored case in full: its plan by name, its request and side arguments over the file's defaults, null pointers of the answer."""
    full = dict(case, plan=_GOLDEN["plans"][case["plan"]], request=dict(_GOLDEN["request_defaults"], **case["request"]))
    if case["side"] is not None:
        full["side"] = dict(_GOLDEN["side_defaults"], **case["side"])
    if case["answer"]["status"] == 0:
        full["answer"] = dict(case["answer"], pointers=[case["answer"]["pointers"].get(n) for n in _GOLDEN["pointer_fields"]])
    return full


CASES = [_expand(c) for c in _GOLDEN["cases"]]


def _names(text):
    return tuple(n for n in text.decode().split(",") if n)


class Harness:
    def __init__(self, so):
        self.so = ctypes.CDLL(so)
        for f in ("request", "side", "keys", "switch", "int", "pointer"):
            fn = getattr(self.so, "count_plan_harness_%s_fields" % f)
            fn.restype = ctypes.c_char_p
            setattr(self, f + "_fields", _names(fn()))
        self.so.count_plan_harness_error.restype = ctypes.c_char_p


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libcount_plan_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "count_plan_harness.cpp")])
    return Harness(so)


@pytest.fixture(scope="module")
def lib():
    from gsn_amd import _abi
    _abi.build()
    return _abi.lib()


def plan_table(spec):
    """The host plan table of a case: gsn_count_plan_build over the case's patterns, then the case's word patches."""
    from gsn_amd.counting import CountPlan
    plan = CountPlan([[tuple(e) for e in p] for p in spec["patterns"]], spec["mode"], spec["induced"], spec["directed_orbits"], spec["directed"],
                     spec["wide"])
    table = plan.table.copy()
    for index, value in spec["patch"]:
        table[index] = value
    return table


def addresses(case):
    """name -> address of every pointer of the case: null, low bits in a slot of its own, or "=name": the address of another pointer."""
    given = {n: case["request"].get(n) for n in POINTERS if "." not in n}
    for group in ("side", "keys"):
        for n in POINTERS:
            if n.startswith(group + "."):
                given[n] = (case[group] or {}).get(n.split(".")[1])
    addr = {n: 0 if v is None else ((i + 1) << 36) + v for i, (n, v) in enumerate(given.items()) if not isinstance(v, str)}
    for n, v in given.items():
        if isinstance(v, str):
            addr[n] = addr[v[1:]]
    return addr


def symbol(address, addr):
    """A pointer of the argument block as the request pointer it equals (the first in POINTERS order), or edge_index + bytes."""
    if address == 0:
        return None
    for n in POINTERS:
        if addr[n] == address:
            return n
    off = address - addr["edge_index"]
    assert addr["edge_index"] and 0 < off < (1 << 35), hex(address)
    return "edge_index+%d" % off


def replay(h, case):
    """Runs the case through the harness; the answer in the golden file's form."""
    addr = addresses(case)
    spec = case["plan"]
    table = None if spec["null"] else np.ascontiguousarray(plan_table(spec), dtype=np.uint32)
    rq = dict(case["request"])
    rq["plan_words"] = spec["words"] if spec["words"] is not None else (0 if table is None else len(table))
    rq_arr = (ctypes.c_int64 * len(h.request_fields))(*[addr[n] if n in addr else rq[n] for n in h.request_fields])

    def group(name, fields):
        if case[name] is None:
            return None
        return (ctypes.c_int64 * len(fields))(*[addr[name + "." + n] if name + "." + n in addr else case[name][n] for n in fields])
    side, keys = group("side", h.side_fields), group("keys", h.keys_fields)
    ncls = None if case["n_classes"] is None else (ctypes.c_int32 * len(case["n_classes"]))(*case["n_classes"])
    assert set(case["switches"]) <= set(h.switch_fields)
    sw = (ctypes.c_char_p * len(h.switch_fields))(*[None if n not in case["switches"] else case["switches"][n].encode() for n in h.switch_fields])
    ints = (ctypes.c_int64 * (len(h.int_fields) + ENC_MAX_COLS))()
    ptrs = (ctypes.c_int64 * len(h.pointer_fields))()
    rc = h.so.count_plan_harness_run(None if table is None else table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), rq_arr, ncls, side, keys, sw, ints, ptrs)
    if rc != 0:
        return {"status": rc, "error": h.so.count_plan_harness_error().decode()}
    assert h.so.count_plan_harness_error() == b""
    n = len(h.int_fields)
    values = list(ints[:n])
    values[h.int_fields.index("kernel")] = KERNELS[values[h.int_fields.index("kernel")]]
    enc_n = list(ints[n:])
    while enc_n and enc_n[-1] == 0:
        enc_n.pop()
    return {"status": 0, "ints": values, "enc_n": enc_n, "pointers": [symbol(p, addr) for p in ptrs]}


def test_field_lists_are_the_recorded_ones(harness):
    """The answers are stored by position: the harness lists the plan's fields in the order they were recorded in."""
    assert list(harness.int_fields) == _GOLDEN["int_fields"]
    assert list(harness.pointer_fields) == _GOLDEN["pointer_fields"]
    assert len(CASES) == len({c["name"] for c in CASES}) >= 100


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_equals_the_recorded_launch(lib, harness, case):
    got = replay(harness, case)
    want = case["answer"]
    if want["status"] == 0 and got["status"] == 0:      # name the fields that differ before the whole answers are compared
        diff = {n: (g, w) for n, g, w in zip(harness.int_fields, got["ints"], want["ints"]) if g != w}
        diff.update({n: (g, w) for n, g, w in zip(harness.pointer_fields, got["pointers"], want["pointers"]) if g != w})
        assert not diff
    assert got == want
