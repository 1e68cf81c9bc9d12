"""The privacy kernels on the GPU (csrc/kernels/privacy.hip through ``ops.kernels.privacy_*`` and
``parallel.privacy.Privatizer``): the norm against fp64 within a derived bound, the clip decision bit
for bit from the device's own norm, ``apply`` at sigma = 0 bitwise against the torch specification,
the Gaussian stream against its fp64 host mirror and its statistics, ``apply`` with noise bitwise
against (the sigma = 0 result) + sigma * ``privacy_gauss``, launch-geometry independence, canaries,
a real model arena, and the binding's refusals.

Noise kernel (ocml logf / sincospif / sqrtf): the measured max |privacy_gauss - torch_gauss| over the
2^20 draws at first4 = 0 and at first4 = 2^32 - 8 is 4.768e-07 = 2^-21 at both (MI355X; recorded in
profiles/privacy_cost.txt): one fp32 ulp of a value in [4, 8).  The test's tolerance is four times that,
1.907e-06; the condition the kernel's math functions must meet is a deviation <= 2e-5."""
import math

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.parallel import (
    privacy as pv)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 4000                                 # 1 000 float4: three full blocks and a partial one
N_WRAP = 4096 * 1024 + 4 * 257           # the 4 096-block grid-stride loop wraps; ragged tail
PADS = (0, 1984, N - 64)                 # 64-float alignment pads: +0 in w and anchor
SEED = 0x5EEDF00DCAFE
GAUSS_DEVIATION = 2e-5                   # the condition on max |device - fp64 mirror|: ~10 x an accurate fp32 libm
GAUSS_TOL = 4 * 2.0 ** -21               # four times the measured deviation (module docstring)


def _make(n, pads, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    anchor = 0.05 * torch.randn(n, device=DEV, generator=g)
    w = anchor + 1e-3 * torch.randn(n, device=DEV, generator=g)
    for p in pads:
        w[p:p + 64] = 0.0
        anchor[p:p + 64] = 0.0
    return w, anchor


@pytest.fixture(scope="module")
def small():
    """(w, anchor) at N; computed once, never written."""
    return _make(N, PADS, 17)


@pytest.fixture(scope="module")
def wrap():
    """(w, anchor) at N_WRAP; computed once, never written."""
    return _make(N_WRAP, (0, 64 * 40001, N_WRAP - 64), 23)


def _norm(w, anchor, clip):
    n = w.numel()
    partial = torch.full((K.privacy_grid(n),), float("nan"), dtype=torch.float64, device=DEV)
    stats = torch.full((4,), -7.0, device=DEV)
    K.privacy_norm(w, anchor, partial, stats, clip)
    return partial, stats


def _i32(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("which", ["small", "wrap"])
def test_norm(which, request):
    w, anchor = request.getfixturevalue(which)
    n = w.numel()
    grid = K.privacy_grid(n)
    assert grid == (4 if n == N else 4096) == K.robust_agg_grid(n)
    partial, stats = _norm(w, anchor, 100.0)
    S = float(partial.sum())                                    # (fp64)
    want = float((w - anchor).double().square().sum())          # fp64 norm^2 of the fp32 differences
    L = math.ceil((n // 4) / (grid * 256))
    # one rounding for d is shared with the reference; two for d * d (d's relative error enters squared),
    # 4L - 1 fp32 additions of non-negative terms; the doubles are negligible
    bound = (4 * L + 4) * 2.0 ** -24
    rel = abs(S - want) / want
    print(f"privacy_norm n={n}: relative error of the sum of squares {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound
    norm32 = torch.tensor(math.sqrt(S), dtype=torch.float64).to(torch.float32)
    ulp = abs(float(torch.nextafter(norm32, torch.tensor(float("inf"))) - norm32))
    assert abs(float(stats[0]) - float(norm32)) <= ulp
    assert stats[1:].tolist() == [1.0, 0.0, 0.0]                # norm (~0.06 / ~2) <= 100: unclipped
    # the clip decision follows bit for bit from the device's own norm
    dn = stats[0].clone()
    for factor in (0.5, 1.0, 2.0, 0.3):                         # (0.3: a division that rounds)
        clip = float(dn) * factor                               # (exact in fp32 at the first three factors)
        _, st = _norm(w, anchor, clip)
        assert torch.equal(_i32(st[0:1]), _i32(dn.view(1)))
        if factor < 1.0:
            scale = (torch.tensor(clip, dtype=torch.float32) / dn.cpu()).view(1)   # IEEE fp32 division, on the host
            assert torch.equal(_i32(st[1:2].cpu()), _i32(scale)) and st[2:].tolist() == [1.0, 0.0]
        else:
            assert st[1:].tolist() == [1.0, 0.0, 0.0]
    # two launches: identical bits
    p2, s2 = _norm(w, anchor, 100.0)
    assert torch.equal(p2.view(torch.int64), partial.view(torch.int64)) and torch.equal(_i32(s2), _i32(stats))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_norm_of_a_nonfinite_update(bad, small):
    w, anchor = small[0].clone(), small[1]
    w[2345] = bad
    _, stats = _norm(w, anchor, 1.0)
    assert not math.isfinite(float(stats[0])) and stats[1:].tolist() == [0.0, 2.0, 0.0]


def _apply(w, anchor, stats, sigma=0.0, shadow=True, round=0, client=0, first4=0, seed=SEED):
    out = w.clone()
    sh = torch.full((w.numel(),), 7.0, dtype=torch.bfloat16, device=DEV) if shadow else None
    K.privacy_apply(out, anchor, sh, stats, sigma, seed, round, client, first4)
    return out, sh


def _stats_for(w, anchor, which):
    """The device's stats for an unclipped (0), clipped (1) or diverged (2) update."""
    if which == 2:
        bad = w.clone()
        bad[7] = float("nan")
        return _norm(bad, anchor, 1.0)[1], bad
    _, st = _norm(w, anchor, 1.0)
    clip = float(st[0]) * (2.0 if which == 0 else 0.25)
    return _norm(w, anchor, clip)[1], w


@pytest.mark.parametrize("which", [0, 1, 2])
def test_apply_without_noise_equals_the_specification(which, small, wrap):
    for w0, anchor in (small, wrap):
        stats, w = _stats_for(w0, anchor, which)
        assert int(stats[2]) == which
        out, sh = _apply(w, anchor, stats)
        want = w.clone()
        rep = pv.torch_privatize_(want, anchor, 1.0, 0.0, stats=stats.tolist())
        assert rep["clipped"] == which
        assert torch.equal(_i32(out), _i32(want))
        assert torch.equal(sh.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))
        if which == 0:
            assert torch.equal(_i32(out), _i32(w))              # identity: not re-rounded
        if which == 2:
            assert torch.equal(_i32(out), _i32(anchor)) and bool(torch.isfinite(out).all())
        if which == 1:
            clip = 0.25 * float(_norm(w, anchor, 1.0)[1][0])
            assert float((out.double() - anchor.double()).norm()) <= clip * (1 + 1e-6)
        out2, _ = _apply(w, anchor, stats, shadow=False)        # without the shadow: the same weights
        assert torch.equal(_i32(out2), _i32(out))


def _gauss(n, round=0, client=0, first4=0, seed=SEED):
    out = torch.full((n,), float("nan"), device=DEV)
    K.privacy_gauss(out, seed, round, client, first4)
    return out


@pytest.mark.parametrize("first4", [0, (1 << 32) - 8])
def test_gauss_against_the_host_mirror(first4):
    """2^20 draws against the fp64 Box-Muller of the same Philox words; at first4 = 2^32 - 8 the
    counter's second word takes over after 8 float4."""
    n = 1 << 20
    got = _gauss(n, 2, 3, first4)
    want = pv.torch_gauss(n, SEED, 2, 3, first4).to(DEV)
    dev = float((got.double() - want.double()).abs().max())
    print(f"privacy_gauss first4={first4}: max |device - fp64 mirror| = {dev:.3e}")
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 5.77
    assert dev <= GAUSS_DEVIATION                               # the condition on the kernel's math functions
    assert dev <= GAUSS_TOL
    assert torch.equal(_i32(_gauss(n, 2, 3, first4)), _i32(got))  # the same arguments: the same bits
    if first4:
        assert torch.equal(_i32(got[32:64]), _i32(_gauss(32, 2, 3, 1 << 32)))


def gauss_statistics(streams):
    """The 5-sigma bounds of tests/test_privacy_cpu.py on three [N] fp64 streams keyed (0, 0), (1, 0),
    (0, 1); returns the figures in units of sigma."""
    figs = {}
    for rc, g in streams.items():
        n = g.numel()
        mean, var = float(g.mean()), float(g.var(unbiased=False))
        kurt = float(((g - mean) ** 4).mean()) / var ** 2
        lag1 = float((g[:-1] * g[1:]).mean())
        figs[rc] = (abs(mean) * math.sqrt(n), abs(var - 1.0) / math.sqrt(2.0 / n),
                    abs(kurt - 3.0) / math.sqrt(24.0 / n), abs(lag1) * math.sqrt(n - 1), float(g.abs().max()))
        assert abs(mean) <= 5.0 / math.sqrt(n), (rc, mean)
        assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / n), (rc, var)
        assert abs(kurt - 3.0) <= 5.0 * math.sqrt(24.0 / n), (rc, kurt)
        assert abs(lag1) <= 5.0 / math.sqrt(n - 1), (rc, lag1)
        assert float(g.abs().max()) <= 5.77, rc
    keys = list(streams)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            a, b = streams[keys[i]], streams[keys[j]]
            cross = float((a * b).mean())
            figs[(keys[i], keys[j])] = abs(cross) * math.sqrt(a.numel())
            assert abs(cross) <= 5.0 / math.sqrt(a.numel()), (keys[i], keys[j], cross)
    return figs


def test_gauss_statistics_and_streams():
    streams = {rc: _gauss(1 << 22, *rc).double().cpu() for rc in ((0, 0), (1, 0), (0, 1))}
    figs = gauss_statistics(streams)
    print("privacy_gauss statistics (units of sigma; max |g| last):", figs)
    base = _gauss(4096, 3, 5)
    for other in (_gauss(4096, 4, 5), _gauss(4096, 3, 6), _gauss(4096, 3, 5, seed=SEED + 1),
                  _gauss(4096, 3, 5, seed=SEED + (1 << 32))):
        assert float((other == base).float().mean()) < 0.01
    assert torch.equal(_i32(_gauss(1024, 3, 5, first4=100)), _i32(base[400:1424]))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_apply_with_noise(which, small, wrap):
    """Bitwise (the sigma = 0 result) + sigma * privacy_gauss, in torch fp32 on the device."""
    sigma = torch.tensor(0.0125, dtype=torch.float32, device=DEV)
    for (w0, anchor), first4 in ((small, 0), (wrap, 12345), (small, (1 << 32) - 8)):
        stats, w = _stats_for(w0, anchor, which)
        base, _ = _apply(w, anchor, stats)
        g = _gauss(w.numel(), 4, 9, first4)
        want = base + sigma * g
        out, sh = _apply(w, anchor, stats, float(sigma), round=4, client=9, first4=first4)
        assert torch.equal(_i32(out), _i32(want)), (which, first4)
        assert torch.equal(sh.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))
        assert not torch.equal(out, base)


def test_launch_geometry_independence(small):
    w, anchor = small
    for which in (0, 1):
        stats, _ = _stats_for(w, anchor, which)
        full, fsh = _apply(w, anchor, stats, 0.0125, round=1, client=2)
        for a, b in ((0, 1024), (1028, 2056), (2052, N), (4, 8)):
            out, sh = _apply(w[a:b], anchor[a:b], stats, 0.0125, round=1, client=2, first4=a // 4)
            assert torch.equal(_i32(out), _i32(full[a:b])), (which, a, b)
            assert torch.equal(sh.view(torch.int16), fsh[a:b].view(torch.int16)), (which, a, b)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_nothing_outside_the_buffers_is_written(which, small):
    """w, shadow, partial and stats sit between 64-element canaries; partial starts as garbage and every
    entry of [0, grid) is overwritten; the anchor is not written."""
    C = 64
    w0, a0 = small
    if which == 2:
        w0 = w0.clone()
        w0[7] = float("inf")
    grid = K.privacy_grid(N)
    wbig = torch.full((N + 2 * C,), 1234.5, device=DEV)
    sbig = torch.full((N + 2 * C,), 7.0, dtype=torch.bfloat16, device=DEV)
    pbig = torch.full((grid + 2 * C,), -77.0, dtype=torch.float64, device=DEV)
    tbig = torch.full((4 + 2 * C,), -5.0, device=DEV)
    abig = torch.full((N + 2 * C,), 99.0, device=DEV)
    w, sh, part, st, anchor = wbig[C:C + N], sbig[C:C + N], pbig[C:C + grid], tbig[C:C + 4], abig[C:C + N]
    w.copy_(w0)
    anchor.copy_(a0)
    clip = {0: 1.0, 1: 0.01, 2: 1.0}[which]
    K.privacy_norm(w, anchor, part, st, clip)
    K.privacy_apply(w, anchor, sh, st, 0.0125, SEED, 1, 2, 0)
    torch.cuda.synchronize()
    for big, n, val in ((wbig, N, 1234.5), (sbig, N, 7.0), (pbig, grid, -77.0), (tbig, 4, -5.0), (abig, N, 99.0)):
        for can in (big[:C], big[C + n:]):
            assert torch.equal(can, torch.full_like(can, val))
    assert torch.equal(anchor, a0)
    assert int(st[2]) == which and float(st[3]) == 0.0
    if which != 2:
        assert bool((part >= 0).all())                           # (no entry keeps its garbage)
        assert float(part.sum()) > 0
    else:
        assert not bool(torch.isfinite(part).all()) and bool((part[1:] >= 0).all())
    assert bool(torch.isfinite(w).all()) and torch.equal(sh.view(torch.int16), w.to(torch.bfloat16).view(torch.int16))


def _batch(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(S // 3, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = ids * mask
    ids[:, 0] = 101
    labels = torch.randint(0, 2, (B,), generator=g)
    return ids.cuda(), mask.cuda(), labels.cuda(), int(lens.sum())


def test_privatizer_on_a_model_arena():
    """``Privatizer.privatize_`` on the default DistilBERT arena: the pads are +0 in master and shadow,
    the shadow the kernel wrote is the shadow a refresh would write, the report matches the
    specification's norm within the norm test's bound, the noise has the configured std, and a graphed
    training step runs on the result."""
    model = DDoSClassifier(device=DEV, impl="hip", seed=3)
    A = model.arena
    anchor = A.master.clone()
    live = torch.zeros(A.numel, dtype=torch.bool, device=DEV)
    for name in A.names():
        off, shape = A.offsets[name]
        live[off:off + math.prod(shape)] = True
    assert int((~live).sum()) == A.numel - A.n_params > 0
    g = torch.Generator(device=DEV).manual_seed(5)
    A.master.add_(1e-4 * torch.randn(A.numel, device=DEV, generator=g) * live)
    trained = A.master.clone()
    want_norm = float((trained - anchor).double().norm())       # ~0.8
    p = pv.Privatizer(clip=0.5, noise_multiplier=0.02, seed=SEED)
    rep = p.privatize_(A.master, anchor, 1, 2, 4, shadow=A.shadow, arena=A)
    model.mark_shadow_synced()
    torch.cuda.synchronize()
    L = math.ceil((A.numel // 4) / (4096 * 256))
    assert abs(rep["update_l2"] - want_norm) / want_norm <= (4 * L + 4) * 2.0 ** -24 / 2 + 2.0 ** -24
    assert rep is p.last and rep["clipped"] == 1 and rep["sigma"] == pv.f32(0.02 * 0.5 / 2.0) == p.sigma(4)
    assert rep["scale"] == float(torch.tensor(0.5) / torch.tensor(rep["update_l2"], dtype=torch.float32))
    assert not A.master[~live].view(torch.int32).any() and not A.shadow[~live].view(torch.int16).any()
    assert torch.equal(A.shadow.view(torch.int16), A.master.to(torch.bfloat16).view(torch.int16))
    # the live weights: the specification fed the device's stats, with the device's own Gaussians
    base = trained.clone()
    pv.torch_privatize_(base, anchor, 0.5, 0.0, stats=[rep["update_l2"], rep["scale"], 1.0])
    noise = (A.master - base)[live].double()
    assert abs(float(noise.std()) / rep["sigma"] - 1.0) < 0.01 and abs(float(noise.mean())) < 5 * rep["sigma"] / 8000
    gs = torch.empty(A.numel, device=DEV)
    K.privacy_gauss(gs, SEED, 2, 1)
    want = base + torch.tensor(rep["sigma"], dtype=torch.float32, device=DEV) * gs
    assert torch.equal(_i32(A.master[live]), _i32(want[live]))
    model.eval()
    ids, mask, labels, tokens = _batch(16, 128, seed=1)
    with torch.no_grad():
        first = model.forward(ids, mask).clone()
        model.sync_shadow(force=True)
        second = model.forward(ids, mask).clone()
    assert torch.isfinite(first).all() and torch.equal(first, second)
    model.train()
    opt = ArenaAdam(model, lr=1e-3)
    opt.reset_state()
    st = GraphedTrainStep(make_step_fn(model, opt), warmup=1, bucket=model.packed_rows)
    before = A.master.clone()
    losses = [float(st(ids, mask, labels, tokens)) for _ in range(3)]
    torch.cuda.synchronize()
    assert st.failed is None and len(st.graphs) >= 1 and all(math.isfinite(v) for v in losses)
    assert not torch.equal(A.master, before)


def test_refusals():
    """The binding rejects each invalid call before any launch: the buffers keep their contents."""
    n = 2048
    mk = lambda k=n, dt=torch.float32: torch.ones(k, dtype=dt, device=DEV)  # noqa: E731
    w, a, sh = mk(), mk(), mk(dt=torch.bfloat16)
    part, st = mk(K.privacy_grid(n), torch.float64), mk(4)
    ext = K.ext()
    ok_norm = dict(w=w, anchor=a, partial=part, stats=st, clip=0.5)
    ok_apply = dict(w=w, anchor=a, shadow=sh, stats=st, sigma=0.01, seed_lo=1, seed_hi=2, round=3, client=4, first4=0)
    ok_gauss = dict(out=w, seed_lo=1, seed_hi=2, round=3, client=4, first4=0)

    def bad(fn, ok, **kw):
        with pytest.raises(RuntimeError):
            getattr(ext, fn)(**dict(ok, **kw))

    big = mk(2 * n)
    for fn, ok in (("privacy_norm", ok_norm), ("privacy_apply", ok_apply)):
        bad(fn, ok, w=mk(dt=torch.float64))                       # dtypes
        bad(fn, ok, anchor=mk(dt=torch.bfloat16))
        bad(fn, ok, stats=mk(4, torch.float64))
        bad(fn, ok, w=mk(2 * n)[::2])                             # not contiguous
        bad(fn, ok, anchor=mk(2 * n)[::2])
        bad(fn, ok, anchor=mk().cpu())                            # another device
        bad(fn, ok, stats=mk(4).cpu())
        bad(fn, ok, w=mk(n - 2), anchor=mk(n - 2), **({"shadow": None} if fn == "privacy_apply" else {}))  # n % 4
        bad(fn, ok, anchor=mk(n - 4))                             # sizes
        bad(fn, ok, stats=mk(3))
        bad(fn, ok, stats=mk(8))
        bad(fn, ok, anchor=w)                                     # anchor is w
        bad(fn, ok, w=big[:n], anchor=big[n // 2:n // 2 + n])     # anchor overlaps w
    bad("privacy_norm", ok_norm, partial=mk(K.privacy_grid(n), torch.float32))
    bad("privacy_norm", ok_norm, partial=mk(K.privacy_grid(n) - 1, torch.float64))   # short partial
    bad("privacy_norm", ok_norm, partial=part.cpu())
    for clip in (0.0, -1.0, float("inf"), float("nan"), 1e300, 1e-300):
        bad("privacy_norm", ok_norm, clip=clip)
    bad("privacy_apply", ok_apply, shadow=mk())                   # fp32 shadow
    bad("privacy_apply", ok_apply, shadow=mk(n - 4, torch.bfloat16))
    bad("privacy_apply", ok_apply, shadow=sh.cpu())
    bad("privacy_apply", ok_apply, w=big[:n], shadow=big[n // 2:n].view(torch.bfloat16))  # shadow overlaps w
    bad("privacy_apply", ok_apply, anchor=big[:n], shadow=big[n // 2:n].view(torch.bfloat16))  # ... or the anchor
    for sigma in (-0.01, float("inf"), float("nan"), 1e300):
        bad("privacy_apply", ok_apply, sigma=sigma)
    for fn, ok in (("privacy_apply", ok_apply), ("privacy_gauss", ok_gauss)):
        for kw in (dict(round=-1), dict(client=-1), dict(first4=-1), dict(round=1 << 32), dict(client=1 << 32),
                   dict(seed_lo=-1), dict(seed_hi=1 << 32)):
            bad(fn, ok, **kw)
    bad("privacy_gauss", ok_gauss, out=mk(n - 2))
    bad("privacy_gauss", ok_gauss, out=mk(dt=torch.float64))
    bad("privacy_gauss", ok_gauss, out=mk(2 * n)[::2])
    with pytest.raises(ValueError):
        K.privacy_gauss(w, 1 << 64, 0, 0)
    torch.cuda.synchronize()
    assert all(torch.equal(t, torch.ones_like(t)) for t in (w, a, sh, part, st, big))
    K.privacy_norm(big[:n], big[n:], part, st, 0.5)               # beside w: accepted
    K.privacy_apply(big[:n], big[n:], sh, st, 0.0, SEED, 0, 0)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0, 1.0, 0.0, 0.0] and torch.equal(big, torch.ones_like(big))
