"""The native dropout on the GPU (gsn_amd/dropout.py, csrc/dropout.hip) against the numpy referee tests/dropout_ref.py, bit for bit: forward
and backward at the sizes around the chunk, the counter bookkeeping, misaligned views, special inputs, the state's interface, HIP-graph
capture, the models' ``dropout_impl="native"`` against the torch path driven by the referee's masks, and the whole training step replayed
with dropout on.  Comparisons are of the fp32 BIT PATTERNS unless a test says otherwise."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import dropout_ref as ref

pytestmark = pytest.mark.gpu
no_capture = pytest.mark.skipif(os.environ.get("PYTORCH_NO_CUDA_MEMORY_CACHING") == "1",
                                reason="stream capture cannot free memory without the caching allocator (scripts/oob_check.sh)")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x9e3779b97f4a7c15          # (bit 63 set: stored two's complement)
PS = (0.1, 0.5, 0.9)


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _gd():
    from gsn_amd import dropout
    return dropout


def _chunk():
    from gsn_amd import _abi
    return int(_abi.lib().gsn_dropout_chunk_elems())


def _signed(v):
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >> 63 else v


def _fresh(seed=SEED, calls=0):
    st = _gd().DropoutState("cuda", seed)
    if calls:
        st.set_state(torch.tensor([_signed(seed), _signed(calls)], dtype=torch.int64))
    return st


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t, dtype=np.float32)
    return a.view(np.uint32)


def _same(got, want, what=""):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %08x vs %08x" % (what, bad.size, g.size, bad[0], g.reshape(-1)[bad[0]],
                                                                                     w.reshape(-1)[bad[0]])


def _call(x, p, res, st):
    """(out, used) of one training call through the autograd node"""
    return _gd()._DropoutFn.apply(x, res, float(p), st)


def _sizes():
    C = _chunk()
    return [1, 2, 3, 4, 5, 7, 8, C - 1, C, C + 1, 2 * C + 3, 3 * C]


@pytest.mark.parametrize("case", list(range(12)) + ["matrix"])
def test_forward_and_backward_against_the_referee(case):
    """Every size around a group and around a chunk, a [37, 300] matrix, p in {0.1, 0.5, 0.9}, with and without a residual: outputs, input
    gradient and residual gradient bit for bit, and after each call state[1] advanced by exactly 1, done == 0, used == (seed, calls before).
    The call counter starts just below 2^32, so the calls cross into the hi32(calls) word of the Philox counter."""
    shape = (37, 300) if case == "matrix" else (_sizes()[case],)
    n = int(np.prod(shape))
    gen = torch.Generator().manual_seed(17 + n)
    c0 = 2 ** 32 - 3
    st = _fresh(SEED, c0)
    calls = c0
    for p in PS:
        for with_res in (False, True):
            x = torch.randn(shape, generator=gen).cuda().requires_grad_(True)
            r = torch.randn(shape, generator=gen).cuda().requires_grad_(True) if with_res else None
            g = torch.randn(shape, generator=gen).cuda()
            out, used = _call(x, p, r, st)
            out.backward(g)
            what = "n=%d p=%g res=%s calls=%d" % (n, p, with_res, calls)
            _same(out, ref.forward(x.detach().cpu().numpy(), None if r is None else r.detach().cpu().numpy(), SEED, calls, p), what + " out")
            _same(x.grad, ref.backward(g.cpu().numpy(), SEED, calls, p), what + " grad_x")
            if with_res:
                _same(r.grad, g, what + " grad_res")
            assert out.shape == x.shape and out.is_contiguous() and not used.requires_grad
            assert used.cpu().tolist() == [_signed(SEED), calls], what
            assert st.get_state().tolist() == [_signed(SEED), calls + 1], what
            assert int(st._done.item()) == 0, what
            calls += 1
    assert calls == c0 + 6 and calls > 2 ** 32


def test_misaligned_views_draw_the_aligned_call():
    """x, res and grad_out at storage offsets of 1, 2 and 3 floats, independently (27 + 27 combinations with the aligned ones): the groups
    are numbered from the tensor's first element, so the bits equal the aligned call's at the same state."""
    C = _chunk()
    n, p, calls = C + 6, 0.5, 11
    gen = torch.Generator().manual_seed(5)
    xb, rb, gb = (torch.randn(n, generator=gen).cuda() for _ in range(3))
    st = _fresh(SEED, calls)
    state0 = st.get_state()
    xa = xb.clone().requires_grad_(True)
    out_a, _ = _call(xa, p, rb, st)
    out_a.backward(gb)
    _same(out_a, ref.forward(xb.cpu().numpy(), rb.cpu().numpy(), SEED, calls, p), "aligned")

    def view(t, off):
        buf = torch.empty(n + 4, device="cuda")
        buf[off:off + n].copy_(t)
        v = buf[off:off + n]
        assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
        return v
    for ox in range(4):
        for orr in range(4):
            for og in range(4):
                if (ox, orr, og) == (0, 0, 0) or 0 in (ox, orr, og) and (ox + orr + og) % 2:      # all 27 misaligned triples, half of the mixed ones
                    continue
                st.set_state(state0)
                x = view(xb, ox).detach().requires_grad_(True)
                out, _ = _call(x, p, view(rb, orr), st)
                out.backward(view(gb, og))
                _same(out, out_a, "offsets %d %d %d out" % (ox, orr, og))
                _same(x.grad, xa.grad, "offsets %d %d %d grad" % (ox, orr, og))
    # without a residual
    st.set_state(state0)
    out_n, _ = _call(xb, p, None, st)
    for ox in (1, 2, 3):
        st.set_state(state0)
        _same(_call(view(xb, ox), p, None, st)[0], out_n, "offset %d, no residual" % ox)
    # a non-contiguous input is made contiguous: the transposed view of the transposed matrix
    m = torch.randn(300, 37, generator=gen).cuda()
    st.set_state(state0)
    want = ref.forward(m.t().contiguous().cpu().numpy(), None, SEED, calls, p)
    _same(_gd().dropout(m.t(), p, True, None, st), want, "non-contiguous")


def test_special_values_do_not_leave_dropped_elements():
    """NaN and +-Inf in dropped and in kept positions (read off the referee's mask): a dropped element is the residual (+0 without one)
    whatever x holds -- a select, not a product with zero; a kept one carries the special value.  Non-NaN elements are compared bit for
    bit; where the referee has a NaN the kernel must have one too (which NaN is the hardware's choice, not the stream's)."""
    n, p, calls = 4099, 0.5, 3
    keep = ref.mask(SEED, calls, n, ref.threshold(p))
    kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
    assert kept.size > 100 and dropped.size > 100
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(n, generator=gen)
    r = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    specials = [float("nan"), float("inf"), float("-inf")]
    for i, v in enumerate(specials * 2):
        x[int(kept[7 * i + 1])] = v
        x[int(dropped[5 * i + 2])] = v
        g[int(kept[3 * i + 40])] = v
        g[int(dropped[3 * i + 41])] = v
    r[int(dropped[0])] = -0.0
    for res in (None, r):
        st = _fresh(SEED, calls)
        xg = x.cuda().requires_grad_(True)
        out, _ = _call(xg, p, None if res is None else res.cuda(), st)
        out.backward(g.cuda())
        for got, want, what in ((out, ref.forward(x.numpy(), None if res is None else res.numpy(), SEED, calls, p), "out"),
                                (xg.grad, ref.backward(g.numpy(), SEED, calls, p), "grad")):
            got = got.detach().cpu().numpy()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), what
            assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what
            assert nan.sum() == 2 and np.isinf(want).sum() == 4, what          # the kept specials arrive ...
            base = np.zeros(n, np.float32) if (res is None or what == "grad") else (res.numpy() + np.float32(0.0))
            assert np.array_equal(got.view(np.uint32)[dropped], base.view(np.uint32)[dropped]), what      # ... the dropped ones leave no trace


def test_host_decided_cases_launch_nothing():
    """p == 0 and eval mode return x (x + residual) and p == 1 zeros (the residual) without a launch; n == 0 launches nothing either: the
    state stays where it was.  Launches are seen through the flags.KERNEL_TIMER hook."""
    from gsn_amd import flags
    gd = _gd()
    st = _fresh(SEED, 7)
    s0 = st.get_state()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(5, 33, generator=gen).cuda().requires_grad_(True)
    r = torch.randn(5, 33, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(5, 33, generator=gen).cuda()
    flags.KERNEL_TIMER = {}
    try:
        for p, training in ((0.0, True), (0.5, False), (0.0, False)):
            assert gd.dropout(x, p, training, None, st) is x
            _same(gd.dropout(x, p, training, r, st), x.detach() + r.detach(), "p=%g training=%s" % (p, training))
        m = gd.Dropout(0.5, state=st).eval()
        assert m(x) is x
        # p == 1: everything dropped
        out = gd.dropout(x, 1.0, True, None, st)
        out.backward(g)
        _same(out, torch.zeros(5, 33), "p=1")
        _same(x.grad, torch.zeros(5, 33), "p=1 grad")
        x.grad = None
        out = gd.dropout(x, 1.0, True, r, st)
        out.backward(g)
        _same(out, r, "p=1 residual")
        _same(x.grad, torch.zeros(5, 33), "p=1 residual grad_x")
        _same(r.grad, g, "p=1 residual grad_res")
        # no elements
        e = torch.empty(0, 7, device="cuda", requires_grad=True)
        out = gd.dropout(e, 0.5, True, None, st)
        assert out.shape == (0, 7)
        out.sum().backward()
        assert e.grad.shape == (0, 7)
        assert "dropout_fwd" not in flags.KERNEL_TIMER and "dropout_bwd" not in flags.KERNEL_TIMER
        assert st.get_state().tolist() == s0.tolist() and int(st._done.item()) == 0
        # and a real call is one launch per direction
        x.grad = None
        gd.dropout(x, 0.5, True, r, st).backward(g)
        assert len(flags.KERNEL_TIMER["dropout_fwd"]) == 1 and len(flags.KERNEL_TIMER["dropout_bwd"]) == 1
        assert st.get_state().tolist() == [s0[0].item(), s0[1].item() + 1]
        # needs_input_grad: no input gradient wanted, no backward launch
        xd = x.detach()
        gd.dropout(xd, 0.5, True, r, st).backward(g)
        assert len(flags.KERNEL_TIMER["dropout_fwd"]) == 2 and len(flags.KERNEL_TIMER["dropout_bwd"]) == 1
    finally:
        flags.KERNEL_TIMER = None
    torch.cuda.synchronize()


def test_state_handling():
    gd = _gd()
    x = torch.randn(1000, generator=torch.Generator().manual_seed(2)).cuda()
    st = gd.DropoutState("cuda", 1234)
    assert st.get_state().tolist() == [1234, 0] and st.get_state().dtype == torch.int64 and not st.get_state().is_cuda
    a, b = gd.dropout(x, 0.5, True, None, st), gd.dropout(x, 0.5, True, None, st)
    assert not torch.equal(a, b)                                   # consecutive calls differ
    _same(a, ref.forward(x.cpu().numpy(), None, 1234, 0, 0.5), "call 0")
    _same(b, ref.forward(x.cpu().numpy(), None, 1234, 1, 0.5), "call 1")
    saved = st.get_state()
    assert saved.tolist() == [1234, 2]
    seq = [gd.dropout(x, 0.3, True, None, st).clone() for _ in range(3)]
    st.set_state(saved)                                            # the same sequence again
    for k, want in enumerate(seq):
        _same(gd.dropout(x, 0.3, True, None, st), want, "after set_state, call %d" % k)
    st.manual_seed(1234)                                           # seed and counter back
    assert st.get_state().tolist() == [1234, 0]
    _same(gd.dropout(x, 0.5, True, None, st), a, "after manual_seed")
    other = gd.DropoutState("cuda", 1235)                           # another seed, another stream
    assert not torch.equal(gd.dropout(x, 0.5, True, None, other), a)
    # the default seed is torch's: torch.manual_seed governs it
    torch.manual_seed(4242)
    assert gd.DropoutState("cuda").get_state().tolist() == [4242, 0]
    d = gd.default_state("cuda")
    assert d is gd.default_state(torch.device("cuda", torch.cuda.current_device())) and d.device.index == torch.cuda.current_device()
    with pytest.raises(ValueError):
        st.set_state(torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        st.set_state(torch.zeros(2, dtype=torch.int32))
    # the module draws from the state it was given
    st.manual_seed(77)
    m = gd.Dropout(0.5, state=st).train()
    _same(m(x, residual=x), ref.forward(x.cpu().numpy(), x.cpu().numpy(), 77, 0, 0.5), "module")


@no_capture
def test_capture_replays_follow_the_device_counter():
    """GraphedStep over dropout(x, p, residual=r) and its backward: replay j equals the referee at calls = c0 + j for four replays (the
    warm-up calls advanced the counter, the capture itself did not), the state afterwards is c0 + 4; a state cannot be created under
    capture."""
    from gsn_amd.graphs import GraphedStep
    gd = _gd()
    C = _chunk()
    n, p = C + 37, 0.5
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, generator=gen).cuda().requires_grad_(True)
    r = torch.randn(n, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(n, generator=gen).cuda()
    st = _fresh(SEED, 100)

    def fn():
        out = gd.dropout(x, p, True, r, st)
        gx, gr = torch.autograd.grad(out, [x, r], g)
        return out, gx, gr
    step = GraphedStep(fn, warmup=2)
    c0 = int(st.get_state()[1])
    assert c0 == 102
    xn, rn, gn = x.detach().cpu().numpy(), r.detach().cpu().numpy(), g.cpu().numpy()
    for j in range(4):
        out, gx, gr = step()
        torch.cuda.synchronize()
        _same(out, ref.forward(xn, rn, SEED, c0 + j, p), "replay %d out" % j)
        _same(gx, ref.backward(gn, SEED, c0 + j, p), "replay %d grad_x" % j)
        _same(gr, g, "replay %d grad_res" % j)
    assert st.get_state().tolist() == [_signed(SEED), c0 + 4] and int(st._done.item()) == 0
    # a refilled input and a state set from the host are both followed by the next replay
    with torch.no_grad():
        x.copy_(torch.randn(n, generator=gen))
    st.set_state(torch.tensor([_signed(SEED), 5], dtype=torch.int64))
    out, gx, gr = step()
    torch.cuda.synchronize()
    _same(out, ref.forward(x.detach().cpu().numpy(), rn, SEED, 5, p), "replay after set_state")
    graph = torch.cuda.CUDAGraph()
    a = torch.zeros(4, device="cuda")
    with torch.cuda.graph(graph):
        b = a + 1
        with pytest.raises(RuntimeError, match="capturing"):
            gd.DropoutState("cuda", 1)
        with pytest.raises(RuntimeError, match="capturing"):
            st.manual_seed(3)
    del b


def _rule_ok(got, want, what):
    """the project's element-wise rule: |got - ref| <= 1e-5 |ref| + 1e-5 max |ref row|"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, what
    if got.dim() < 2:
        got, want = got.reshape(1, -1), want.reshape(1, -1)
    got, want = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    bound = 1e-5 * want.abs() + 1e-5 * want.abs().amax(dim=1, keepdim=True)
    excess = ((got - want).abs() - bound).max().item() if got.numel() else 0.0
    print("%s: worst |got - ref| - bound = %.3g (max |ref| %.3g)" % (what, excess, want.abs().max().item() if want.numel() else 0.0))
    assert excess <= 0.0, "%s: off by %.3g beyond the bound" % (what, excess)


def _models(kind, impl):
    """(model, forward closure) of the builders of scripts/, small: GNN_OGB with residual and virtual node, GNNSubstructures, DGNNet"""
    dev = torch.device("cuda", 0)
    if kind == "ogb":
        m = _script("train_step_molhiv")
        args = types.SimpleNamespace(batch=32, layers=3, d=64, optimizer="sgd", activation="elu", dropout=impl, residual=True)
        model, data, params, opt, loss_of, N, E = m.build(args, dev, 0, dropout=0.5)
        assert model.residual and model.vn and model.dropout_impl == impl
        return model, (lambda: model(data))
    if kind == "zinc":
        m = _script("train_step_zinc")
        # every layer's representation is projected: the jumping-knowledge sum has five terms, four of them with the sum so far as residual
        args = types.SimpleNamespace(batch=48, optimizer="sgd", activation="elu", dropout=impl, dropout_p=0.5, final_projection=[True] * 5)
        model, data, params, opt, loss_of, N, E = m.build(args, dev, 0)
        assert model.dropout_impl == impl and model.dropout_features[0] == 0.5 and all(model.final_projection)
        return model, (lambda: model(data))
    from gsn_amd import dgn
    m = _script("bench_dgn")
    b, ef_np, codes_np = m.batch(32)
    g = dgn.DGNGraph.from_batch(b, edge_field=ef_np)
    torch.manual_seed(0)
    net = m.make_net(impl, dropout=0.3, in_feat_dropout=0.2)
    assert net.dropout_impl == impl and all(l.dropout_impl == impl for l in net.layers)
    codes = torch.from_numpy(codes_np).cuda()
    return net, (lambda: net(g, codes, None, g.snorm_n, None))


@pytest.mark.parametrize("kind", ["ogb", "zinc", "dgn"])
def test_models_with_native_dropout_against_the_torch_path_on_the_referees_masks(kind, monkeypatch):
    """dropout_impl="native" in train mode under set_state(s) against the same model with "torch", whose F.dropout is replaced by the
    referee's masks in call order c0, c0 + 1, ...: outputs and every parameter gradient within the project's element-wise rule (the models'
    adjoints accumulate with float atomics: not bitwise).  In eval mode the two implementations give the same bits."""
    import torch.nn.functional as F
    gd = _gd()
    seed, c0 = 0x1234567887654321, 2 ** 32 - 2
    torch.manual_seed(0)
    native, fwd_native = _models(kind, "native")
    torch.manual_seed(0)
    plain, fwd_plain = _models(kind, "torch")
    for (ka, a), (kb, b) in zip(native.state_dict().items(), plain.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    st = gd.default_state("cuda")
    st.set_state(torch.tensor([seed, c0], dtype=torch.int64))
    native.train()
    y = fwd_native()
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(8)).cuda()
    (y * w).sum().backward()
    n_calls = int(st.get_state()[1]) - c0
    assert n_calls > 0

    counter = [c0]

    def referee_dropout(input, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return input
        keep = torch.from_numpy(ref.mask(seed, counter[0], input.numel(), ref.threshold(p))).reshape(input.shape).to(input.device)
        counter[0] += 1
        return torch.where(keep, input * float(ref.scale(p)), torch.zeros((), device=input.device))
    monkeypatch.setattr(F, "dropout", referee_dropout)
    plain.train()
    yr = fwd_plain()
    (yr * w).sum().backward()
    monkeypatch.undo()
    assert counter[0] - c0 == n_calls, "the two paths call dropout %d and %d times" % (n_calls, counter[0] - c0)
    _rule_ok(y, yr, kind + " output")
    checked = 0
    for (name, pa), (_, pb) in zip(native.named_parameters(), plain.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), name
        if pa.grad is not None:
            _rule_ok(pa.grad, pb.grad, kind + " grad " + name)
            checked += 1
    assert checked > 4
    native.eval()
    plain.eval()
    s0 = st.get_state()
    with torch.no_grad():
        _same(fwd_native(), fwd_plain(), kind + " eval")
    assert st.get_state().tolist() == s0.tolist()


def _eager_step(opt, loss_of):
    opt.zero_grad(set_to_none=True)
    loss = loss_of()
    loss.backward()
    opt.step()
    return loss.detach()


def _rel(sa, sb):
    """tests/test_graphed_train_gpu.py's measure: max over the floating-point tensors of max|a - b| / max(max|a|, 1 % of the state's largest)"""
    scale = max(float(v.double().abs().max()) for v in sa.values() if v.is_floating_point() and v.numel())
    worst = 0.0
    for k in sa:
        if sa[k].is_floating_point():
            den = max(float(sa[k].double().abs().max()), 0.01 * scale)
            worst = max(worst, float((sa[k].double() - sb[k].double()).abs().max()) / den)
        else:
            assert torch.equal(sa[k], sb[k]), k
    return worst


def _train_run(n_steps, warm, lr, state):
    """State and losses of the molhiv B = 32 step with native dropout 0.5 after n_steps from dropout state `state` (all eager when warm is
    None; else `warm` eager warm-up steps inside GraphedTrainStep, then replays)."""
    from gsn_amd.graphs import GraphedTrainStep
    gd = _gd()
    torch.manual_seed(1234)
    m = _script("train_step_molhiv")
    args = types.SimpleNamespace(batch=32, layers=3, d=64, optimizer="sgd", activation="elu", dropout="native")
    model, data, params, opt, loss_of, N, E = m.build(args, torch.device("cuda", 0), 0, dropout=0.5)
    assert model.dropout_impl == "native"
    for g in opt.param_groups:
        g["lr"] = lr
    st = gd.default_state("cuda")
    st.set_state(state)
    if warm is None:
        losses = [float(_eager_step(opt, loss_of)) for _ in range(n_steps)]
    else:
        step = GraphedTrainStep(loss_of, opt, params, warmup=warm)
        losses = [None] * warm + [float(step()) for _ in range(n_steps - warm)]
    torch.cuda.synchronize()
    calls = int(st.get_state()[1]) - int(state[1])
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, losses, calls


@no_capture
def test_graphed_train_step_with_native_dropout():
    """The molhiv B = 32 step with dropout 0.5, native.  With lr = 0 the replays' losses differ (every replay reads the advanced counter).
    From one dropout state, eager steps on one copy and warm-up + replays on a twin draw the same masks: the losses agree within the bound
    tests/test_graphed_train_gpu.py derives for replay == eager -- the run-to-run noise of the eager steps' float atomics, measured here on
    two eager runs, times the same factors (state: max(16 noise, 2e-5); loss: max(64 noise, 1e-3) relative + 1e-7)."""
    state = torch.tensor([99, 2 ** 32 - 4], dtype=torch.int64)
    _, frozen, _ = _train_run(6, 2, 0.0, state)
    assert len(set(frozen[2:])) > 1, "every replay drew the same dropout masks: %r" % (frozen,)
    n_steps, warm = 4, 2
    sa, la, ca = _train_run(n_steps, None, 3e-3, state)
    sa2, la2, _ = _train_run(n_steps, None, 3e-3, state)
    sb, lb, cb = _train_run(n_steps, warm, 3e-3, state)
    assert ca == cb and ca > 0 and ca % n_steps == 0, (ca, cb)          # the same number of dropout calls per step, eager or replayed
    noise = _rel(sa, sa2)
    diff = _rel(sa, sb)
    print("eager run-to-run %.3g, replay against eager %.3g; losses eager %r, eager again %r, replayed %r" % (noise, diff, la, la2, lb))
    assert diff <= max(16.0 * noise, 2e-5), "replays drift from eager: %.3g (eager run-to-run: %.3g)" % (diff, noise)
    for x, y in zip(la[warm:], lb[warm:]):
        assert abs(x - y) <= max(64.0 * noise, 1e-3) * abs(x) + 1e-7, "loss %.6g vs %.6g" % (x, y)
