"""CPU checks of the native dropout (gsn_amd/dropout.py, csrc/dropout.hip): the numpy referee tests/dropout_ref.py against the known answers
of Philox4x32-10, the threshold and scale constants, the stream of gsn_amd/csrc/dropout_core.h run on the host by the stand-alone program
tests/dropout_harness.cpp (built with the address and undefined-behaviour sanitizers, run as a process) against the referee, the refusals
decided on the host, and the new symbols of the built library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import dropout_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_referee_known_answers():
    for counter, key, want in KNOWN:
        got = ref.philox4x32_10(counter, key)
        assert tuple(int(w) for w in got) == want
    # vectorised over counters: the same words as one call at a time
    got = ref.philox4x32_10(([0, 0x243f6a88], [0, 0x85a308d3], [0, 0x13198a2e], [0, 0x03707344]), ([0, 0xa4093822], [0, 0x299f31d0]))
    assert [tuple(int(w[i]) for w in got) for i in range(2)] == [k[2] for k in KNOWN]


def test_referee_mask_is_the_single_element_rule():
    seed, calls, thr = 0x8123456789abcdef, 5, ref.threshold(0.3)
    for n in (1, 3, 4, 5, 9, 64):
        m = ref.mask(seed, calls, n, thr)
        assert m.shape == (n,) and np.array_equal(m, ref.keep_at(seed, calls, np.arange(n), thr))
    assert np.array_equal(ref.mask(seed, calls, 64, thr)[:9], ref.mask(seed, calls, 9, thr))       # (no dependence on the size)
    assert not np.array_equal(ref.mask(seed, calls, 64, thr), ref.mask(seed, calls + 1, 64, thr))
    share = ref.mask(1, 0, 1 << 16, ref.threshold(0.3)).mean()
    assert abs(share - 0.7) < 0.01


def test_threshold_and_scale():
    from gsn_amd import dropout as gd
    ps = [0.0, 1e-12, 1e-6, 0.1, 0.25, 0.3, 0.5, 0.75, 0.9, 0.999999, 1.0 - 2.0 ** -33, 1.0 - 2.0 ** -40, 1.0]
    th = [ref.threshold(p) for p in ps]
    assert th == sorted(th) and th[0] == 0
    assert ref.threshold(0.5) == 2 ** 31
    assert ref.threshold(1.0) == 2 ** 32 - 1 and ref.threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1 and ref.threshold(1.0 - 2.0 ** -33) == 2 ** 32 - 1
    assert all(0 <= t <= 2 ** 32 - 1 for t in th)
    for p in ps:
        assert gd.threshold(p) == ref.threshold(p)
    for p in (0.1, 0.25, 0.3, 0.5, 0.9):
        s = gd.scale(p)
        assert np.float32(s) == ref.scale(p) and float(np.float32(s)) == s          # a float32 value, the double division rounded once
    assert gd.scale(0.5) == 2.0 and gd.scale(0.9) == float(np.float32(1.0 / (1.0 - 0.9)))


def _cases():
    thr = [ref.threshold(0.1), ref.threshold(0.5), ref.threshold(0.9), 0, 2 ** 32 - 1]
    seeds = [0, 1, 0x8000000000000000, 0xffffffffffffffff, 0xdeadbeef00000001, 0x7fffffffffffffff]
    calls = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 + 5]
    es = [0, 1, 2, 3, 4, 7, 8191, 8192, 2 ** 32 - 1, 2 ** 32, 2 ** 34 - 4, 2 ** 34 - 1, 2 ** 34, 2 ** 34 + 1, 2 ** 34 + 4, 2 ** 40 + 3]
    out = []
    for i, e in enumerate(es):
        for j, c in enumerate(calls):
            out.append((seeds[(i + j) % len(seeds)], c, e, thr[(i + 2 * j) % len(thr)]))
    for s in seeds:
        out.append((s, 3, 5, thr[1]))
    return out


def test_stream_on_host_under_sanitizers():
    """csrc/dropout_core.h -- Philox4x32-10, the counter and key layout, the word of an element, the keep rule -- by a stand-alone program:
    the two known answers, and the keep decision and word of every case against the referee.  The cases hold e on both sides of 2^34 (the
    hi32(q) word of the counter), calls on both sides of 2^32, and seeds with their high bits set."""
    exe = os.path.join(REPO, "tests", "_build", "dropout_harness")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(REPO, "tests", "dropout_harness.cpp")])
    cases = _cases()
    assert any(e < 2 ** 34 for _, _, e, _ in cases) and any(e >= 2 ** 34 for _, _, e, _ in cases)
    assert any(c < 2 ** 32 for _, c, _, _ in cases) and any(c >= 2 ** 32 for _, c, _, _ in cases) and any(s >> 63 for s, _, _, _ in cases)
    r = subprocess.run([exe] + ["%x" % v for case in cases for v in case], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("dropout harness ok") and len(lines) == 1 + len(cases)
    kept = 0
    for line, (seed, calls, e, thr) in zip(lines[1:], cases):
        f = line.split()
        assert [int(v, 16) for v in f[:4]] == [seed, calls, e, thr], line
        want = bool(ref.keep_at(seed, calls, [e], thr)[0])
        q = e >> 2
        word = int(ref.philox4x32_10((q & 0xffffffff, q >> 32, calls & 0xffffffff, calls >> 32), (seed & 0xffffffff, seed >> 32))[e & 3])
        assert int(f[5], 16) == word and int(f[4]) == int(want) == int(word >= thr), line
        kept += want
    assert 0 < kept < len(cases)


def test_refusals_on_the_host():
    """Decided in front of any launch: this runs with or without a GPU."""
    from gsn_amd import dropout as gd
    x = torch.zeros(4, 3)
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="between 0 and 1"):
            gd.dropout(x, p)
        with pytest.raises(ValueError, match="between 0 and 1"):
            gd.Dropout(p)
    for dt in (torch.float64, torch.float16, torch.int64):
        with pytest.raises(TypeError, match="float32"):
            gd.dropout(x.to(dt), 0.5)
    with pytest.raises(TypeError, match="residual must be float32"):
        gd.dropout(x, 0.5, residual=x.double())
    with pytest.raises(ValueError, match="residual of shape"):
        gd.dropout(x, 0.5, residual=torch.zeros(3, 4))
    # a CPU tensor: the error gsn_amd.evaluation raises for one (RuntimeError, "no CPU fallback"), in train and in eval mode
    from gsn_amd import evaluation
    with pytest.raises(RuntimeError, match="no CPU fallback") as want:
        evaluation.masked_loss("L1Loss", x, x)
    for training in (True, False):
        with pytest.raises(RuntimeError, match="no CPU fallback") as got:
            gd.dropout(x, 0.5, training=training)
        assert type(got.value) is type(want.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gd.DropoutState("cpu")
    with pytest.raises(ValueError, match="dropout_impl"):
        gd.resolve_impl("cuda")
    assert gd.resolve_impl("torch") == "torch" and gd.resolve_impl("native") == "native"


def test_flag_and_default_implementation(monkeypatch):
    from gsn_amd import dropout as gd, flags
    assert flags.DROPOUT_NATIVE == (os.environ.get("GSN_DROPOUT", "torch") == "native")
    monkeypatch.setattr(flags, "DROPOUT_NATIVE", False)
    assert gd.resolve_impl(None) == "torch"
    monkeypatch.setattr(flags, "DROPOUT_NATIVE", True)
    assert gd.resolve_impl(None) == "native"


def test_symbols_in_the_built_library():
    from gsn_amd import _abi
    _abi.build()
    raw = ctypes.CDLL(os.path.join(REPO, "gsn_amd", "lib", "libgsn_hip.so"))
    for name in ("gsn_dropout_fwd_hip", "gsn_dropout_bwd_hip", "gsn_dropout_chunk_elems"):
        assert hasattr(raw, name) and name in _abi.SIGNATURES, name
    lib = _abi.lib()
    hdr = open(os.path.join(REPO, "include", "gsn_abi.h")).read()
    import re
    chunk = int(re.search(r"#define GSN_DROPOUT_CHUNK_ELEMS (\d+)", hdr).group(1))
    assert lib.gsn_dropout_chunk_elems() == chunk and chunk % 1024 == 0
    # refused or ignored on the host, without a launch: no elements, a negative count, null pointers
    assert lib.gsn_dropout_fwd_hip(0, None, None, None, 1, 1.0, None, None, None, None) == 0
    assert lib.gsn_dropout_bwd_hip(0, None, None, 1, 1.0, None, None) == 0
    assert lib.gsn_dropout_fwd_hip(-1, None, None, None, 1, 1.0, None, None, None, None) != 0
    assert lib.gsn_dropout_fwd_hip(4, None, None, None, 1, 1.0, None, None, None, None) != 0
    assert lib.gsn_dropout_bwd_hip(4, None, None, 1, 1.0, None, None) != 0
    assert b"gsn_dropout_bwd_hip" in lib.gsn_last_error()
