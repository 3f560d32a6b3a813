"""The optimizer step of csrc/optim.hip through the C ABI - gdmae_grad_sq_norm, gdmae_sum_partials(_gated), gdmae_adam_step(_shadow) -
and FlatAdamOneCycle end to end, against the float64 reference, the rounding bound and the crafted inputs of
tests/optimizer_reference.py.  tests/test_optimizer_reference_cpu.py validates that reference and shows that each wrong variant of
the step (decay after the update, eps before the bias division, bias corrections with t - 1, clip from the un-averaged norm, a
decayed gap, a skipped last element, elements beyond the first grid sweep untouched, a truncated shadow) lands >= 5 x outside the
bound used here.

Norm: exact.  Data from {-1, 0, 1} make every partial sum an integer below 2^24, so any summation order gives the count of
non-zeros; a lone 1 at each end, on both sides of the float4 body's end and at the first float of every 262 144-float4 slot
must give exactly 1, one index at a time; the float after the end holds a NaN (a prefetch lane that is clamped but not masked
would show it).  Sizes around the float4 body / scalar tail and around the 4 194 304-float sweep; an unaligned base (scalar path).
One rounded case (normal data, n = 9 000 003) against float64 at NORM_CHAIN = 45 roundings x 2^-24 (the count is written out in
optimizer_reference.py).
Adam: every parameter set of optimizer_reference.PARAM_SETS on single segments [0, n) around the 256-thread block and the
1 048 576-element grid sweep, and on the segment lists (odd ends, touching, empty ones in between, a short segment before / after a
1.2 M one, 64 segments).  p', m', v' inside bounds() around step_f64; outside the segments p, m, v and the shadow keep their bits
(the shadow is pre-filled with a pattern); the shadow equals p'.bfloat16() in bits; gdmae_adam_step gives the same bits as the
shadow variant, and so does a second run.  Exact by construction and asserted as equalities: gradients x 8 with grad_scale 1/8
and sq_norm x 64; p' = p on the shadow's rounding edges; rejected calls leave the buffers alone.
FlatAdamOneCycle: 20 steps of a 2 904-element module (two buckets, one frozen tensor between the two Adam segments) against the
float64 run, bound 4 x d_ref (d_ref = oracle.optim_oracle.AdamOneCycle in float32 on the CPU against float64, floor 1e-7 of the
tensor's largest entry; the oracle has no notion of frozen parameters, so the frozen tensor is put back after each of its steps and
its gradient still counts in the norm); shadows after every step; resume from state_dict() after step 10 and the four-rank
averaging are bit-identical.  The four-rank step goes through all_reduce_grads with world_size patched to 4 and GradSync in its
documented mode "off" (no process group exists in a one-process test, so no collective can run; the averaging is what is checked).

Nothing is fitted to the kernel's output.  Each test prints bound and measured error per tensor.
Measured (MI355X): profiles/optimizer_step_reference.txt.  Every equality holds.  Worst measured / bound:
  norm, normal data, n = 9 000 003     0.002  (relative error 4.047e-09, bound 45 x 2^-24 = 2.682e-06)
  Adam, single segments   p' 0.287  ([0,2500001) t2-clip-gs8: 2.745e-07 / 9.575e-07)   m' 0.495   v' 0.498  ([0,2500001))
  Adam, segment lists     p' 0.286  (short-long t100000-nonorm: 2.758e-07 / 9.651e-07)  m' 0.494   v' 0.496  (short-long t1-clip)
  (step_f32, the float32 numpy evaluation on the CPU, reaches 0.27 / 0.49 / 0.47 of the same bounds)
  FlatAdamOneCycle        0.295 of 4 x d_ref (b.lin.weight, step 16: error 3.917e-07, d_ref 3.321e-07); d_ref at step 19:
                          a.weight 4.770e-07, a.bias 2.976e-07, b.lin.weight 4.314e-07, b.lin.bias 2.157e-07, c.weight 2.444e-07,
                          c.bias 7.799e-08; elsewhere 0.250: the device's and the float32 oracle's largest errors coincide to the printed digits
No defect was found: csrc/optim.hip, k_sum_partials and gdmae_hip/optim.py are unchanged by these tests.
"""
import functools
import math

import numpy as np
import pytest
import torch

import optimizer_reference as R
from gdmae_hip import configs, optim
from gdmae_hip import lib as L
from oracle import optim_oracle as oo

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5          # shadow pre-fill: a bf16 NaN pattern no update produces (+ index % 7, see _sentinel)


def _dev():
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _sentinel(n):
    return (SENTINEL + np.arange(n) % 7).astype(np.uint16)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------------
# norm
# ---------------------------------------------------------------------------------------------------------------------------
def _sq_norm(buf, n, part, out, k=0):
    """gdmae_grad_sq_norm of buf[:n] into out[k] (no synchronisation)"""
    assert 0 < n <= buf.numel() and part.numel() >= 1024 and k < out.numel()
    L.call("gdmae_grad_sq_norm", buf.data_ptr(), n, L.ptr(part), out.data_ptr() + 4 * k, L.stream())


@functools.lru_cache(maxsize=None)
def _zeros():
    """one zeroed buffer for the planted-value checks of all sizes (every test leaves it zeroed)"""
    return torch.zeros(max(R.NORM_SIZES) + 2, dtype=torch.float32, device=_dev())


@pytest.mark.parametrize("n", R.NORM_SIZES)
def test_grad_sq_norm_is_exact_on_integer_data_and_sees_every_planted_value(n):
    d = _dev()
    host = np.random.default_rng(n).integers(-1, 2, n + 1).astype(np.float32)
    host[n] = np.nan                                              # past the end: must not enter the sum, masked or not
    g = torch.from_numpy(host).to(d)
    part = torch.full((1024,), np.nan, dtype=torch.float32, device=d)
    idx = R.planted_indices(n)
    out = torch.full((1 + len(idx),), -1.0, dtype=torch.float32, device=d)
    _sq_norm(g, n, part, out, 0)
    z = _zeros()
    z[n] = float("nan")
    for k, i in enumerate(idx):
        z[i] = 1.0
        _sq_norm(z, n, part, out, 1 + k)
        z[i] = 0.0
    z[n] = 0.0
    got = out.cpu().numpy()
    want = float(np.count_nonzero(host[:n]))
    print(f"norm n={n}: sum {got[0]:.0f} (exact {want:.0f}); planted at {idx}: {got[1:].tolist()}")
    assert got[0] == want
    assert (got[1:] == 1.0).all(), [i for i, x in zip(idx, got[1:]) if x != 1.0]


def test_grad_sq_norm_unaligned_base_takes_the_scalar_path_to_the_same_answer():
    d, n = _dev(), 100003
    host = np.random.default_rng(3).integers(-1, 2, n + 2).astype(np.float32)
    host[0] = host[n + 1] = np.nan                                # on both sides of the view
    buf = torch.from_numpy(host).to(d)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    part = torch.empty(1024, dtype=torch.float32, device=d)
    out = torch.full((4,), -1.0, dtype=torch.float32, device=d)
    _sq_norm(view, n, part, out, 0)
    aligned = torch.from_numpy(host[1:n + 1].copy()).to(d)
    assert aligned.data_ptr() % 16 == 0
    _sq_norm(aligned, n, part, out, 1)
    buf[1:n + 1] = 0.0
    for k, i in enumerate((0, n - 1)):
        view[i] = 1.0
        _sq_norm(view, n, part, out, 2 + k)
        view[i] = 0.0
    got = out.cpu().numpy()
    print(f"norm unaligned n={n}: {got.tolist()}")
    assert got[0] == got[1] == float(np.count_nonzero(host[1:n + 1])) and got[2] == got[3] == 1.0


def test_grad_sq_norm_rounded_data_within_the_chain_bound():
    d, n = _dev(), 9000003
    host = np.random.default_rng(11).standard_normal(n).astype(np.float32)
    g = torch.from_numpy(host).to(d)
    part = torch.empty(1024, dtype=torch.float32, device=d)
    out = torch.zeros(2, dtype=torch.float32, device=d)
    _sq_norm(g, n, part, out, 0)
    _sq_norm(g, n, part, out, 1)
    got = out.cpu().numpy().astype(np.float64)
    ref = float(np.square(host.astype(np.float64)).sum())
    bound = R.NORM_CHAIN * R.U * (1.0 + R.NORM_CHAIN * R.U)
    rel = abs(got[0] - ref) / ref
    print(f"norm rounded n={n}: relative error {rel:.3e}, bound {bound:.3e} ({R.NORM_CHAIN} roundings), measured / bound {rel / bound:.3f}")
    assert rel <= bound and got[0] == got[1]


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000])
def test_sum_partials_and_its_gated_form_are_exact_on_integers(n):
    d = _dev()
    host = np.random.default_rng(n).integers(-3, 4, n + 1).astype(np.float32)
    host[n] = np.nan
    part = torch.from_numpy(host).to(d)
    s = float(host[:n].astype(np.float64).sum())
    out = torch.full((8,), 7.0, dtype=torch.float32, device=d)
    gate = torch.tensor([0.5, 0.25, 0.125, float("nan")], dtype=torch.float32, device=d)
    st = L.stream()
    L.call("gdmae_sum_partials", L.ptr(part), n, 1.0, out.data_ptr(), 0, st)
    L.call("gdmae_sum_partials", L.ptr(part), n, 0.25, out.data_ptr() + 4, 0, st)
    L.call("gdmae_sum_partials", L.ptr(part), n, 0.25, out.data_ptr() + 8, 1, st)
    L.call("gdmae_sum_partials", L.ptr(part), n, -2.0, out.data_ptr() + 12, 1, st)
    for k in range(4):          # gate above gate_min, equal to it (>= passes), below it, NaN
        L.call("gdmae_sum_partials_gated", L.ptr(part), n, 0.25, out.data_ptr() + 16 + 4 * k, gate.data_ptr() + 4 * k, 0.25, st)
    got = out.cpu().numpy().tolist()
    want = [s, 0.25 * s, 7.0 + 0.25 * s, 7.0 - 2.0 * s, 0.25 * s, 0.25 * s, 0.0, 0.0]
    print(f"sum_partials n={n}: {got} (exact {want})")
    assert got == want


# ---------------------------------------------------------------------------------------------------------------------------
# Adam through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def _adam(p, g, m, v, segments, kw, entry="gdmae_adam_step_shadow", rejected=False):
    """one call on fresh device copies of the float32 host arrays: returns (p', m', v', shadow bits, p'.bfloat16() bits, g) on the
    host.  ``rejected``: the entry must return an error (nothing is launched then: it checks its arguments first)."""
    d = _dev()
    n = p.size
    assert rejected or all(0 <= b <= e <= n for b, e in segments)      # the entry checks 0 <= begin <= end; the length is the caller's
    tp, tg, tm, tv = (torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in (p, g, m, v))
    sq = torch.tensor([kw["sq_norm"]], dtype=torch.float32, device=d)
    flat = [x for s in segments for x in s]
    args = [L.ptr(tp), L.ptr(tg), L.ptr(tm), L.ptr(tv), L.host_i64(flat), len(segments), kw["lr"], kw["beta1"], kw["beta2"], kw["eps"],
            kw["wd"], kw["t"], kw["max_norm"], kw["grad_scale"], L.ptr(sq)]
    sh = None
    if entry == "gdmae_adam_step_shadow":
        sh = torch.from_numpy(_sentinel(n).view(np.int16)).to(d)
        args.append(L.ptr(sh))
    if rejected:
        with pytest.raises(L.GdmaeHipError):
            L.call(entry, *args, L.stream())
    else:
        L.call(entry, *args, L.stream())
    return (tp.cpu().numpy(), tm.cpu().numpy(), tv.cpu().numpy(), None if sh is None else _u16(sh),
            _u16(tp.bfloat16().view(torch.int16)), tg.cpu().numpy())


def _check_adam(label, c):
    p2, m2, v2, sh, cast, g2 = _adam(c.p, c.g, c.m, c.v, c.segments, c.ps.kw)
    ins, out = c.inside, ~c.inside
    assert np.array_equal(_bits(g2), _bits(c.g))
    for name, got, old, ref, bnd in zip("pmv", (p2, m2, v2), (c.p, c.m, c.v), c.ref, c.bounds):
        assert np.array_equal(_bits(got)[out], _bits(old)[out]), f"{label}: {name} changed outside the segments"
        err = np.abs(got.astype(np.float64) - ref)[ins]
        assert np.isfinite(err).all(), (label, name)
        q = err / bnd[ins]
        k = int(np.argmax(q))
        print(f"adam {label} {name}': worst measured / bound {q[k]:.3f} (error {err[k]:.3e}, bound {bnd[ins][k]:.3e}); "
              f"largest error {err.max():.3e}, largest bound {bnd[ins].max():.3e}")
        assert q[k] <= 1.0, (label, name, float(q[k]), int(np.flatnonzero(ins)[k]))
    assert np.array_equal(sh[out], _sentinel(c.n)[out]), f"{label}: shadow written outside the segments"
    assert np.array_equal(sh[ins], cast[ins]) and np.array_equal(sh[ins], R.bf16_bits(p2)[ins]), f"{label}: shadow bits"
    again = _adam(c.p, c.g, c.m, c.v, c.segments, c.ps.kw)
    plain = _adam(c.p, c.g, c.m, c.v, c.segments, c.ps.kw, entry="gdmae_adam_step")
    for name, a, b, e in zip("pmv", (p2, m2, v2), again[:3], plain[:3]):
        assert np.array_equal(_bits(a), _bits(b)), f"{label}: {name} differs between two runs"
        assert np.array_equal(_bits(a), _bits(e)), f"{label}: {name} differs between gdmae_adam_step and the shadow variant"
    assert np.array_equal(sh, again[3])
    return p2, m2, v2, sh


@pytest.mark.parametrize("ps_name", [ps.name for ps in R.PARAM_SETS])
@pytest.mark.parametrize("n", R.SINGLE_SIZES)
def test_adam_single_segment(n, ps_name):
    _check_adam(f"[0,{n}) {ps_name}", R.case(n, ps_name, ((0, n),)))


@pytest.mark.parametrize("ps_name", [ps.name for ps in R.PARAM_SETS])
@pytest.mark.parametrize("lst", list(R.SEGMENT_LISTS))
def test_adam_segment_lists(lst, ps_name):
    n, seg = R.SEGMENT_LISTS[lst]
    _check_adam(f"{lst} {ps_name}", R.case(n, ps_name, tuple(seg)))


@pytest.mark.parametrize("ps_name", [ps.name for ps in R.PARAM_SETS if ps.kw["grad_scale"] == 1.0])
@pytest.mark.parametrize("lst", ["odd", "short-long"])
def test_adam_gradients_times_8_with_grad_scale_one_eighth_give_the_same_bits(lst, ps_name):
    """power-of-two scaling is exact through the square root and the products (sq_norm x 64 for the norm of 8 g)"""
    n, seg = R.SEGMENT_LISTS[lst]
    c = R.case(n, ps_name, tuple(seg))
    assert c.ps.kw["grad_scale"] == 1.0
    base = _adam(c.p, c.g, c.m, c.v, c.segments, c.ps.kw)
    kw8 = {**c.ps.kw, "grad_scale": 0.125, "sq_norm": c.ps.kw["sq_norm"] * 64.0}
    g8 = c.g * np.float32(8.0)
    assert np.array_equal(g8 / np.float32(8.0), c.g)
    scaled = _adam(c.p, g8, c.m, c.v, c.segments, kw8)
    for name, a, b in zip(("p", "m", "v", "shadow"), base[:4], scaled[:4]):
        assert np.array_equal(_bits(a), _bits(b)), (lst, ps_name, name)
    assert not np.array_equal(_bits(base[0]), _bits(c.p))


def test_adam_rejected_calls_return_an_error_and_leave_the_buffers_alone():
    n, seg = R.SEGMENT_LISTS["odd"]
    c = R.case(n, "t1-clip", tuple(seg))
    bad = {"65 segments": dict(segments=[(10 * k, 10 * k + 5) for k in range(65)]),
           "begin < 0": dict(segments=[(-1, 5)]),
           "end < begin": dict(segments=[(5, 3)]),
           "a bad segment after a good one": dict(segments=[(0, 5), (7, 6)]),
           "step = 0": dict(segments=c.segments, t=0)}
    for what, ch in bad.items():
        kw = {**c.ps.kw, "t": ch.get("t", c.ps.kw["t"])}
        p2, m2, v2, sh, _, _ = _adam(c.p, c.g, c.m, c.v, ch["segments"], kw, rejected=True)
        for name, got, old in zip("pmv", (p2, m2, v2), (c.p, c.m, c.v)):
            assert np.array_equal(_bits(got), _bits(old)), (what, name)
        assert np.array_equal(sh, _sentinel(n)), what
        print(f"rejected: {what}")


def test_adam_shadow_rounding_edges():
    """g = m = v = 0 and wd = 0: p' = p in bits (ties with an even / odd upper bit, +-0, denormals, the largest finite float), and the
    shadow is its round-to-nearest-even bf16"""
    kw = R.PARAM_SET["t2-total-eq-max"].kw
    assert kw["wd"] == 0.0
    k = R.SHADOW_EDGE_BITS.size
    n = k + 5
    p = np.full(n, 1.5, dtype=np.float32)
    p[2:2 + k] = R.SHADOW_EDGE_BITS.view(np.float32)
    zero = np.zeros(n, dtype=np.float32)
    p2, m2, v2, sh, cast, _ = _adam(p, zero, zero, zero, [(2, 2 + k)], kw)
    print("shadow edges: p bits " + " ".join(f"{x:08x}" for x in _bits(p2)[2:2 + k]))
    print("shadow edges: shadow " + " ".join(f"{x:04x}" for x in sh[2:2 + k]))
    print("shadow edges: expect " + " ".join(f"{x:04x}" for x in R.SHADOW_EDGE_EXPECT))
    assert np.array_equal(_bits(p2), _bits(p))
    assert not _bits(m2).any() and not _bits(v2).any()
    assert np.array_equal(sh[2:2 + k], R.SHADOW_EDGE_EXPECT) and np.array_equal(sh[2:2 + k], cast[2:2 + k])
    assert np.array_equal(sh[:2], _sentinel(n)[:2]) and np.array_equal(sh[2 + k:], _sentinel(n)[2 + k:])


# ---------------------------------------------------------------------------------------------------------------------------
# FlatAdamOneCycle end to end
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = 20


class _Mixed(torch.nn.Module):
    """``w`` sits on a module that has a child: the reference's leaf-module rule leaves it frozen"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(200))
        self.lin = torch.nn.Linear(30, 40)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(40, 30)
        self.b = _Mixed()
        self.c = torch.nn.Linear(17, 13)


def _bucket_of(name):
    return "second" if name.startswith("c.") else "first"


def _fresh(values=None):
    """the crafted module on the device with seeded (or the given) parameter values, and its optimizer"""
    net = _Net()
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.3 if values is None else values[name])
    net = net.to(_dev())
    opt = optim.FlatAdamOneCycle(net, configs.optimization_cfg(), total_steps=STEPS, bucket_of=_bucket_of)
    return net, opt


def _grads(t):
    """fixed gradients of step t per parameter name (CPU float32); every third step is large enough for the clip"""
    gen = torch.Generator().manual_seed(100 + t)
    scale = 1.0 if t % 3 == 1 else 0.05
    return {name: torch.randn(p.shape, generator=gen) * scale for name, p in _Net().named_parameters()}


def _snap(opt):
    return tuple(_bits(x.cpu().numpy()).copy() for x in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)) + (_u16(opt.flat_param_bf16.view(torch.int16)).copy(),)


def _set_grads(net, opt, t, mult=1.0):
    opt.zero_grad()
    g = _grads(t)
    for name, p in net.named_parameters():
        p.grad.copy_((g[name] * mult).to(p.device))


@functools.lru_cache(maxsize=None)
def _run():
    """the uninterrupted 20-step run on the device (bits after every step), the float64 reference run and the float32 oracle run"""
    net, opt = _fresh()
    names = {id(p): n for n, p in net.named_parameters()}
    order = [names[id(p)] for p in opt.params]                        # the flat layout
    frozen = [names[id(p)] for p in opt.frozen]
    assert frozen == ["b.w"] and [b for b, _, _ in opt.buckets] == ["first", "second"]
    assert opt.segments == [0, 2470, 2670, 2904] and opt.n == 2904
    seg = list(zip(opt.segments[0::2], opt.segments[1::2]))
    init = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
    sizes = [init[n].numel() for n in order]
    cat = lambda dct: np.concatenate([dct[n].numpy().reshape(-1) for n in order])
    p64, m64, v64 = cat(init).astype(np.float64), np.zeros(opt.n), np.zeros(opt.n)
    ora_p = [init[n].clone().requires_grad_(True) for n in order]
    ora = oo.AdamOneCycle(ora_p, wd=0.01, max_norm=10.0)
    c = opt.cfg
    snaps, rows, state10, values10, clipped = [], [], None, None, 0
    for t in range(STEPS):
        _set_grads(net, opt, t)
        opt.step()
        snaps.append(_snap(opt))
        # shadows and the frozen tensor after every step
        for n, p in net.named_parameters():
            assert torch.equal(p._gd_shadow[0].view(torch.int16), p.data.bfloat16().view(torch.int16)), (t, n)
            if n in frozen:
                assert torch.equal(p.data.cpu(), init[n]) and torch.equal(p._gd_shadow[0].cpu(), init[n].bfloat16()), (t, n)
        if t == 9:
            state10 = opt.state_dict()
            values10 = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
        # float64 reference and float32 oracle on the same gradients
        g = _grads(t)
        lr, b1 = optim.one_cycle(t, STEPS, c.LR, list(c.MOMS), c.DIV_FACTOR, c.PCT_START)
        g64 = cat(g).astype(np.float64)
        sq = float((g64 * g64).sum())
        clipped += math.sqrt(sq) > 10.0
        p64, m64, v64 = R.step_f64(p64, g64, m64, v64, seg, lr=lr, beta1=b1, beta2=0.99, eps=1e-8, wd=c.WEIGHT_DECAY, t=t + 1,
                                   max_norm=float(c.GRAD_NORM_CLIP), grad_scale=1.0, sq_norm=sq)
        for q, n in zip(ora_p, order):
            q.grad = g[n].clone()
        ora.step(*oo.one_cycle(t, STEPS, c.LR, list(c.MOMS), c.DIV_FACTOR, c.PCT_START))
        with torch.no_grad():
            for q, n in zip(ora_p, order):
                if n in frozen:
                    q.copy_(init[n])
        gpu = snaps[-1][0].view(np.float32).astype(np.float64)
        off = 0
        for q, n, k in zip(ora_p, order, sizes):
            ref = p64[off:off + k]
            d_ref = float(np.abs(q.detach().numpy().reshape(-1).astype(np.float64) - ref).max())
            rows.append((t, n, float(np.abs(gpu[off:off + k] - ref).max()), d_ref, float(np.abs(ref).max())))
            off += k
    assert 0 < clipped < STEPS                                       # the clip is active on some steps only
    return dict(snaps=snaps, rows=rows, state10=state10, values10=values10, frozen=frozen, init=init)


def test_flat_adam_trajectory_within_four_times_the_float32_oracles_error():
    r = _run()
    worst = (0.0, None)
    for t, n, err, d_ref, big in r["rows"]:
        bound = max(4.0 * d_ref, 1e-7 * big)
        print(f"flat_adam step {t:2d} {n:12s}: error {err:.3e}, d_ref {d_ref:.3e}, bound {bound:.3e}, measured / bound {err / bound:.3f}")
        worst = max(worst, (err / bound, (t, n)))
    print(f"flat_adam worst measured / bound {worst[0]:.3f} at step, tensor {worst[1]}")
    for t, n, err, d_ref, big in r["rows"]:
        if n in r["frozen"]:
            assert err == 0.0 and d_ref == 0.0
        assert err <= max(4.0 * d_ref, 1e-7 * big), (t, n, err, d_ref)


def test_flat_adam_resumes_bit_identically_from_its_state_dict():
    r = _run()
    net, opt = _fresh(r["values10"])
    opt.load_state_dict(r["state10"])
    assert opt.t == 10
    for t in range(10, STEPS):
        _set_grads(net, opt, t)
        opt.step()
        for name, a, b in zip(("p", "m", "v", "shadow"), _snap(opt), r["snaps"][t]):
            assert np.array_equal(a, b), (t, name)


def test_flat_adam_four_rank_average_equals_the_plain_step_in_bits(monkeypatch):
    r = _run()
    net, opt = _fresh()
    opt.sync.mode = "off"                    # no process group in a one-process test: no collective, the averaging is what is checked
    monkeypatch.setattr(opt, "world_size", lambda: 4)
    for t in range(3):                       # step 1 has the clip active
        _set_grads(net, opt, t, mult=4.0)      # the SUM over four ranks that hold the same gradient
        opt.all_reduce_grads()
        assert opt._grad_scale == 0.25
        opt.step()
        assert opt._grad_scale == 1.0
        for name, a, b in zip(("p", "m", "v", "shadow"), _snap(opt), r["snaps"][t]):
            assert np.array_equal(a, b), (t, name)
