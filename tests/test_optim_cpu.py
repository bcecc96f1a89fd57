"""Native Adam without a GPU (gsn_amd/optim.py): the float64 referee of the GPU tests pinned to torch, the chunk table of the launch,
state-dict interchange with torch.optim.Adam, what the constructor refuses, and setup_optimization."""
import io
import os
import re

import numpy as np
import pytest
import torch

from adam_ref import adam_ref, normalised_error
from gsn_amd import optim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _signed_log_uniform(gen, shape, lo, hi, dtype):
    mag = torch.exp(torch.empty(shape, dtype=torch.float64).uniform_(np.log(lo), np.log(hi), generator=gen))
    sign = torch.where(torch.rand(shape, generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0)
    return (mag * sign).to(dtype)


@pytest.mark.parametrize("wd", [0.0, 3e-6, 1e-2])
@pytest.mark.parametrize("decoupled", [False, True])
def test_referee_is_torch_in_float64(wd, decoupled):
    """torch.optim.Adam / AdamW (float64, CPU, foreach=False, two groups, 5 steps) against tests/adam_ref.py: every step, fed with
    torch's own previous state, within 2^-46 of the referee in the referee's scales."""
    gen = torch.Generator().manual_seed(5)
    shapes = [(7, 9), (33,), (), (5, 4, 3)]
    params = [torch.nn.Parameter(_signed_log_uniform(gen, s, 1e-3, 10.0, torch.float64)) for s in shapes]
    hyper = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd), dict(lr=3e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=wd / 2)]
    groups = [dict(params=params[:2], **hyper[0]), dict(params=params[2:], **hyper[1])]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(groups, foreach=False)
    worst = 0.0
    for t in range(1, 6):
        before = []
        for i, p in enumerate(params):
            st = opt.state.get(p, {})
            before.append((p.detach().clone(), st["exp_avg"].clone() if st else torch.zeros_like(p), st["exp_avg_sq"].clone() if st else torch.zeros_like(p)))
            p.grad = _signed_log_uniform(gen, p.shape, 1e-6, 100.0, torch.float64)
        opt.step()
        for i, p in enumerate(params):
            h = hyper[0] if i < 2 else hyper[1]
            (rp, rm, rv), (sp, sm, sv) = adam_ref(before[i][0], p.grad, before[i][1], before[i][2], t, h["lr"], h["betas"][0], h["betas"][1],
                                                  h["eps"], h["weight_decay"], decoupled)
            st = opt.state[p]
            assert float(st["step"]) == t
            worst = max(worst, normalised_error(p, rp, sp), normalised_error(st["exp_avg"], rm, sm), normalised_error(st["exp_avg_sq"], rv, sv))
    print("torch float64 vs referee: worst normalised error %.3g = %.1f * 2^-53" % (worst, worst * 2.0 ** 53))
    assert worst <= 2.0 ** -46


def test_chunk_size_mirrors_the_header():
    hdr = open(os.path.join(REPO, "include", "gsn_abi.h")).read()
    assert int(re.search(r"#define\s+GSN_ADAM_CHUNK_ELEMS\s+(\d+)", hdr).group(1)) == optim.CHUNK_ELEMS
    assert int(re.search(r"#define\s+GSN_ADAM_TENSOR_WORDS\s+(\d+)", hdr).group(1)) == optim._TENSOR_WORDS
    assert int(re.search(r"#define\s+GSN_ADAM_GROUP_DOUBLES\s+(\d+)", hdr).group(1)) == optim._GROUP_DOUBLES


def test_chunk_table_covers_every_element_once():
    C = optim.CHUNK_ELEMS
    sizes = [0, 1, 3, 4, 5, C - 1, C, C + 1, 3 * C + 2]
    table = optim.chunk_table(sizes)
    assert table.dtype == np.int32 and table.ndim == 2 and table.shape[1] == 2
    hits = [np.zeros(n, dtype=np.int64) for n in sizes]
    for t, first in table:
        assert 0 <= t < len(sizes) and 0 <= first < sizes[t] and first % C == 0      # starts inside its tensor: it cannot cross into another
        hits[t][first:min(first + C, sizes[t])] += 1
    assert all((h == 1).all() for h in hits)
    assert 0 not in set(table[:, 0].tolist())                                         # the empty tensor has no chunk
    assert table.shape[0] == sum((n + C - 1) // C for n in sizes)
    assert optim.chunk_table([]).shape == (0, 2) and optim.chunk_table([0, 0]).shape == (0, 2)


def _stepped_torch_adam(n_steps=3, **kw):
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in [(4, 6), (), (9,), (3,)]]
    opt = torch.optim.Adam([dict(params=params[:2]), dict(params=params[2:], lr=0.02, betas=(0.8, 0.9), eps=1e-6)], weight_decay=1e-3, **kw)
    for _ in range(n_steps):
        for p in params[:3]:                    # params[3] never receives a gradient
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return params, opt


def _assert_same_state_dicts(a, b, group_keys_of=None):
    assert set(a["state"]) == set(b["state"])
    for k in a["state"]:
        assert set(a["state"][k]) == set(b["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(a["state"][k]["step"]) == float(b["state"][k]["step"])
        assert torch.equal(a["state"][k]["exp_avg"], b["state"][k]["exp_avg"])
        assert torch.equal(a["state"][k]["exp_avg_sq"], b["state"][k]["exp_avg_sq"])
    assert len(a["param_groups"]) == len(b["param_groups"])
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert set(ga) == set(gb)
        for k in ga:
            assert ga[k] == gb[k], k


def test_state_dict_interchange_with_torch():
    params, topt = _stepped_torch_adam()
    tsd = topt.state_dict()
    assert set(topt.defaults) == set(optim.Adam(params).defaults)
    native = optim.Adam([dict(params=params[:2]), dict(params=params[2:])])
    assert native.state_dict()["state"] == {}                      # lazy: nothing has had a gradient yet
    views = [native.flat_state()[0].data_ptr(), native.flat_state()[1].data_ptr()]
    native.load_state_dict(tsd)
    nsd = native.state_dict()
    _assert_same_state_dicts(tsd, nsd)
    assert 3 not in nsd["state"] and params[3] not in native.state  # never had a gradient: absent
    st = native.state[params[0]]
    assert st["step"].dim() == 0 and st["step"].dtype == torch.float32
    exp_avg, exp_avg_sq, steps = native.flat_state()
    assert [exp_avg.data_ptr(), exp_avg_sq.data_ptr()] == views     # load_state_dict copied into the flat buffers ...
    assert st["exp_avg"].data_ptr() == exp_avg.data_ptr() and st["step"].data_ptr() == steps.data_ptr()      # ... and state still views them
    # capturable-style dict (steps as fp32 tensors): same result
    _, topt_c = _stepped_torch_adam()
    csd = topt_c.state_dict()
    for s in csd["state"].values():
        s["step"] = torch.tensor(float(s["step"]), dtype=torch.float32)
    native2 = optim.Adam([dict(params=params[:2]), dict(params=params[2:])])
    native2.load_state_dict(csd)
    _assert_same_state_dicts(tsd, native2.state_dict())
    # torch.save / torch.load round trip
    buf = io.BytesIO()
    torch.save(nsd, buf)
    buf.seek(0)
    native3 = optim.Adam([dict(params=params[:2]), dict(params=params[2:])])
    native3.load_state_dict(torch.load(buf))
    _assert_same_state_dicts(nsd, native3.state_dict())
    # and back into torch: it steps on from the native dict exactly as from its own
    back = torch.optim.Adam([dict(params=params[:2]), dict(params=params[2:])])
    back.load_state_dict(native3.state_dict())
    _assert_same_state_dicts(tsd, back.state_dict())
    for p in params[:3]:
        p.grad = torch.ones_like(p)
    back.step()
    assert float(back.state[params[0]]["step"]) == 4.0
    # a state dict is a copy: it does not move with the optimizer's buffers
    keep = nsd["state"][0]["exp_avg"].clone()
    native.flat_state()[0].add_(1.0)
    assert torch.equal(nsd["state"][0]["exp_avg"], keep)


def test_add_param_group_keeps_state():
    params, topt = _stepped_torch_adam()
    native = optim.Adam([dict(params=params[:2]), dict(params=params[2:])])
    native.load_state_dict(topt.state_dict())
    before = native.state_dict()
    extra = torch.nn.Parameter(torch.zeros(5, 2))
    native.add_param_group(dict(params=[extra], lr=0.5))
    after = native.state_dict()
    assert len(after["param_groups"]) == 3 and after["param_groups"][2]["lr"] == 0.5 and after["param_groups"][2]["params"] == [4]
    after["param_groups"].pop()
    _assert_same_state_dicts(before, after)
    st = native.state[params[2]]
    assert st["exp_avg"].data_ptr() >= native.flat_state()[0].data_ptr() and extra not in native.state


def test_refusals():
    w = torch.nn.Parameter(torch.zeros(4, 4))
    with pytest.raises(ValueError, match="amsgrad"):
        optim.Adam([w], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.Adam([w], maximize=True)
    with pytest.raises(ValueError, match="differentiable"):
        optim.Adam([w], differentiable=True)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.Adam([dict(params=[w], amsgrad=True)])
    with pytest.raises(TypeError, match=r"index 1 of group 0.*float16"):
        optim.Adam([w, torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))])
    with pytest.raises(TypeError, match=r"index 0 of group 0, shape \(4, 2\).*not contiguous"):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, 4)[:, ::2])])
    with pytest.raises(TypeError, match="'layer.weight'"):
        optim.Adam([("layer.weight", torch.nn.Parameter(torch.zeros(2, dtype=torch.float64)))])
    ok = optim.Adam([w])
    with pytest.raises(TypeError):
        ok.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))]))
    assert len(ok.param_groups) == 1
    tsd = torch.optim.Adam([w], amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        ok.load_state_dict(tsd)
    assert ok.defaults["capturable"] is True


def test_step_without_a_gpu_raises_and_updates_nothing():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    w = torch.nn.Parameter(torch.ones(4, 4))
    opt = optim.Adam([w], lr=0.1)
    w.grad = torch.ones(4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(w.detach(), torch.ones(4, 4)) and w._version == 0
    assert float(opt.flat_state()[2].sum()) == 0.0 and float(opt.flat_state()[0].abs().sum()) == 0.0
    w.grad = torch.ones(4, 4).to_sparse()
    with pytest.raises(RuntimeError):
        opt.step()


def test_setup_optimization():
    model = torch.nn.Linear(3, 2)
    opt, sched = optim.setup_optimization(model, lr=1e-2, regularization=1e-4, scheduler="StepLR", decay_steps=2, decay_rate=0.5)
    assert isinstance(opt, optim.Adam) and isinstance(sched, torch.optim.lr_scheduler.StepLR)
    assert opt.param_groups[0]["lr"] == 1e-2 and opt.param_groups[0]["weight_decay"] == 1e-4
    assert sched.step_size == 2 and sched.gamma == 0.5
    opt, sched = optim.setup_optimization(model, lr=1e-2, regularization=0.0, scheduler="ReduceLROnPlateau", decay_rate=0.25, patience=7)
    assert isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau) and sched.factor == 0.25 and sched.patience == 7 and sched.mode == "min"
    sched2 = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.25, patience=0)
    sched2.step(1.0)
    sched2.step(2.0)
    assert opt.param_groups[0]["lr"] == pytest.approx(2.5e-3)       # the scheduler only reads and writes param_groups
    opt, sched = optim.setup_optimization(model, lr=1e-2, regularization=0.0, scheduler="None")
    assert isinstance(opt, optim.Adam) and sched is None
    with pytest.raises(NotImplementedError, match="^Scheduler Cosine is not currently supported.$"):
        optim.setup_optimization(model, lr=1e-2, regularization=0.0, scheduler="Cosine")


def test_entry_argument_checks_under_host_sanitizers(tmp_path):
    """tests/adam_args_main.cpp: a stand-alone program (its own main, no Python) over the argument checks of gsn_adam_step_hip, host code
    compiled with AddressSanitizer and UndefinedBehaviorSanitizer.  Every call returns before a device is touched, so it runs without one.
    (The chunk table is built in Python -- test_chunk_table_covers_every_element_once -- and has no host C++ to sanitize.)"""
    import shutil
    import subprocess
    if torch.cuda.is_available():
        pytest.skip("GPU present: sanitized programs run on machines without one")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "adam_args")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=undefined", os.path.join(REPO, "gsn_amd", "csrc", "optim.hip"),
                    os.path.join(REPO, "tests", "adam_args_main.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 failures" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
