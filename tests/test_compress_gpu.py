"""The quantization kernels on the GPU (csrc/kernels/compress.hip through ``ops.kernels.quant_*`` and
``parallel.compress.Compressor``): encode bit for bit against the torch specification (payload and
residual) at a small length and at one where the grid-stride loop wraps with a ragged last sweep,
crafted groups, the stats against fp64 within a derived bound, decode_mean bit for bit, a slice with
``first``, canaries, run-to-run determinism, a real model arena, and the binding's refusals.

The specification runs on the CPU (IEEE fp32 division, one rounding per operation); no input relies on
denormals."""
import math

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.parallel import (
    compress as cp)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 2048                                  # 32 groups: two blocks at int8, one at int4
N_WRAP = 2 * 4096 * 1024 + 64 * 5         # a multiple of 64, not of 256: the 4 096-block loop wraps at both widths
#                                           (int8: two sweeps + 80 lanes; int4: one sweep + 40 lanes)
SEED = 0x5EEDF00DCAFE


def _make(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    anchor = 0.05 * torch.randn(n, device=DEV, generator=g)
    w = anchor + 1e-3 * torch.randn(n, device=DEV, generator=g) * torch.rand(n, device=DEV, generator=g)
    e = 1e-5 * torch.randn(n, device=DEV, generator=g)
    for p in (0, n - 64):                 # 64-float alignment pads: +0 in w, anchor and residual
        w[p:p + 64] = 0.0
        anchor[p:p + 64] = 0.0
        e[p:p + 64] = 0.0
    return w, anchor, e


@pytest.fixture(scope="module")
def small():
    """(w, anchor, residual) at N, on the device and on the host; computed once, never written."""
    t = _make(N, 17)
    return t, tuple(x.cpu() for x in t)


@pytest.fixture(scope="module")
def wrap():
    t = _make(N_WRAP, 23)
    return t, tuple(x.cpu() for x in t)


def _i32(t):
    return t.view(torch.int32)


def _encode(w, a, e, bits, rounding="nearest", round=0, client=0, first=0, seed=SEED):
    n = w.numel()
    payload = torch.full((K.quant_words(n, bits),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    partial = torch.full((3 * K.quant_grid(n),), float("nan"), dtype=torch.float64, device=DEV)
    stats = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    res = None if e is None else e.clone()
    K.quant_encode(w, a, res, payload, partial, stats, bits, rounding == "stochastic", seed, round, client, first)
    return payload, res, stats, partial


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
@pytest.mark.parametrize("bits", [8, 4])
def test_encode_equals_the_specification(bits, rounding, feedback, small, wrap):
    for (w, a, e), (wc, ac, ec) in (small, wrap):
        n = w.numel()
        assert K.quant_words(n, bits) == cp.payload_words(n, bits)
        assert K.quant_grid(n) == K.privacy_grid(n) == (2 if n == N else 4096)
        payload, res, stats, _ = _encode(w, a, e if feedback else None, bits, rounding, 3, 1)
        want_e = ec.clone() if feedback else None
        want, rep = cp.torch_quantize_(wc, ac, want_e, bits, rounding, SEED, 3, 1)
        assert torch.equal(payload.cpu(), want)
        if feedback:
            assert torch.equal(_i32(res.cpu()), _i32(want_e))
        up, er, bad, zero = stats.tolist()
        assert bad == 0.0 and zero == 0.0 and rep["bad_groups"] == 0
        assert abs(up - rep["update_l2"]) <= 2.0 ** -23 * up and abs(er - rep["error_l2"]) <= 2.0 ** -23 * er
        q, s = cp.split_payload(want, n, bits)
        assert int(q.abs().max()) == cp.QMAX[bits] and not q[:64].any() and not q[-64:].any()
        assert not _i32(s[:1]).any() and not _i32(s[-1:]).any()       # pads: scale +0, codes 0


@pytest.mark.parametrize("bits", [8, 4])
def test_crafted_groups(bits):
    G = 10
    n = 64 * G
    g = torch.Generator().manual_seed(3)
    a = 0.05 * torch.randn(n, generator=g)
    w = a + 1e-3 * torch.randn(n, generator=g)
    e = torch.zeros(n)
    w[0:64] = a[0:64]                                   # 0: all zero
    w[64:128] = a[64:128]
    w[64 + 37] += 0.25                                  # 1: one nonzero element
    w[128] = a[128] - 0.5                               # 2: the maximum in the first lane, negative
    w[192 + 63] = a[192 + 63] - 0.5                     # 3: the maximum in the last lane, negative
    w[256:320], a[256:320] = 1e-3 * torch.randn(64, generator=g), 0.0
    w[256 + 11] = 3e38                                  # 4: 3e38
    w[320 + 5] = float("nan")                           # 5: NaN
    w[384 + 60] = float("inf")                          # 6: inf
    w[448 + 1] = float("-inf")                          # 7: -inf, and a NaN beside it
    w[448 + 2] = float("nan")
    w[512:576], a[512:576] = 3e38, -3e38                # 8: w - anchor overflows
    #                                                     9: an ordinary group
    for rounding in ("nearest", "stochastic"):
        payload, res, stats, _ = _encode(w.to(DEV), a.to(DEV), e.to(DEV), bits, rounding, 1, 2)
        want_e = e.clone()
        want, rep = cp.torch_quantize_(w, a, want_e, bits, rounding, SEED, 1, 2)
        assert torch.equal(payload.cpu(), want) and torch.equal(_i32(res.cpu()), _i32(want_e))
        assert rep["bad_groups"] == 4 and stats[2].item() == 4.0
        q, s = cp.split_payload(payload.cpu(), n, bits)
        q, qm = q.view(G, 64), cp.QMAX[bits]
        assert not q[0].any() and not _i32(s[0:1]).any()
        assert q[1, 37] == qm and int(q[1].abs().sum()) == qm
        assert q[2, 0] == -qm and q[3, 63] == -qm and q[4, 11] == qm
        assert not q[5:9].any() and not _i32(s[5:9]).any()
        assert bool(torch.isfinite(res).all()) and not _i32(res[320:576]).any()      # bad groups: residual +0
        assert float(s[4]) == float(torch.tensor(3e38) / torch.tensor(float(qm))) and bool(q[9].any())
        up, er = stats[0].item(), stats[1].item()
        assert math.isfinite(up) and abs(up - rep["update_l2"]) <= 2.0 ** -23 * up
        assert abs(er - rep["error_l2"]) <= 2.0 ** -23 * er


@pytest.mark.parametrize("which", ["small", "wrap"])
def test_stats(which, request):
    """|v| and |e'| against fp64.  The device squares in fp64 (exact for fp32 inputs) and adds n
    non-negative doubles in a fixed order; so does the reference, in another order: the two sums of
    squares agree within 2 n 2^-53, their roots within half that, and the fp32 roundings of two roots
    that close are at most one ulp apart.  bad_groups is exact."""
    (w, a, e), _ = request.getfixturevalue(which)
    n = w.numel()
    w = w.clone()
    bad = [3, n // 64 - 2] + ([40001] if n == N_WRAP else [])
    for k, g in enumerate(bad):
        w[64 * g + 13 * k] = float("nan") if k % 2 == 0 else float("inf")
    for bits in (8, 4):
        payload, res, stats, partial = _encode(w, a, e, bits)
        good = torch.ones(n // 64, dtype=torch.bool, device=DEV)
        good[bad] = False
        v = ((w - a) + e).view(-1, 64)[good].double()
        up, er, nb, zero = stats.tolist()
        assert nb == float(len(bad)) and zero == 0.0
        p = partial.view(-1, 3)
        assert bool(torch.isfinite(p).all()) and float(p[:, 2].sum()) == float(len(bad))
        for got, S, ref in ((up, float(p[:, 0].sum()), v), (er, float(p[:, 1].sum()), res.view(-1, 64)[good].double())):
            want = float(ref.square().sum())
            rel = abs(S - want) / want
            print(f"quant_encode int{bits} n={n}: relative error of a sum of squares {rel:.3e} (bound {2 * n * 2.0 ** -53:.3e})")
            assert rel <= 2 * n * 2.0 ** -53
            r32 = torch.tensor(math.sqrt(want), dtype=torch.float64).to(torch.float32)
            ulp = abs(float(torch.nextafter(r32, torch.tensor(float("inf"))) - r32))
            assert abs(got - float(r32)) <= ulp and got == float(torch.tensor(got).float())


@pytest.fixture(scope="module")
def payloads(small):
    """16 payloads per width at N (CPU specification), computed once."""
    (_, _, _), (wc, ac, _) = small
    out = {}
    for bits in (8, 4):
        ps = []
        for c in range(16):
            g = torch.Generator().manual_seed(100 + c)
            wk = ac + (1e-3 * (c + 1)) * torch.randn(N, generator=g)
            wk[:64] = 0.0
            ps.append(cp.torch_quantize_(wk, ac, None, bits, "stochastic" if c % 2 else "nearest", SEED, 0, c)[0])
        out[bits] = ps
    return out


@pytest.mark.parametrize("M", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("bits", [8, 4])
def test_decode_mean_equals_the_specification(bits, M, small, payloads):
    (_, a, _), (_, ac, _) = small
    ps = payloads[bits][:M]
    for shadow in (True, False):
        out = torch.full((N,), 7.0, device=DEV)
        sh = torch.full((N,), 7.0, dtype=torch.bfloat16, device=DEV) if shadow else None
        K.quant_decode_mean([p.to(DEV) for p in ps], a, out, sh, bits)
        want, wsh = torch.empty(N), torch.empty(N, dtype=torch.bfloat16)
        cp.torch_decode_mean_(ps, ac, want, wsh, bits)
        assert torch.equal(_i32(out.cpu()), _i32(want))
        if shadow:
            assert torch.equal(sh.cpu().view(torch.int16), wsh.view(torch.int16))
        assert not _i32(out[:64]).any()                           # the pad stays +0
    if M >= 2:                                                    # the order of the payloads is the order of the sum
        out2 = torch.empty(N, device=DEV)
        K.quant_decode_mean([p.to(DEV) for p in reversed(ps)], a, out2, None, bits)
        want2 = torch.empty(N)
        cp.torch_decode_mean_(list(reversed(ps)), ac, want2, None, bits)
        assert torch.equal(_i32(out2.cpu()), _i32(want2))


def test_decode_mean_wrap(wrap):
    """decode_mean where the grid-stride loop wraps, M = 2: round trip of two encodes."""
    (w, a, e), (wc, ac, ec) = wrap
    for bits in (8, 4):
        p0, _, _, _ = _encode(w, a, e, bits)
        p1, _, _, _ = _encode(w, a, None, bits, "stochastic", 1, 1)
        out = torch.empty(N_WRAP, device=DEV)
        sh = torch.empty(N_WRAP, dtype=torch.bfloat16, device=DEV)
        K.quant_decode_mean([p0, p1], a, out, sh, bits)
        want, wsh = torch.empty(N_WRAP), torch.empty(N_WRAP, dtype=torch.bfloat16)
        cp.torch_decode_mean_([p0.cpu(), p1.cpu()], ac, want, wsh, bits)
        assert torch.equal(_i32(out.cpu()), _i32(want)) and torch.equal(sh.cpu().view(torch.int16), wsh.view(torch.int16))


@pytest.mark.parametrize("bits", [8, 4])
def test_a_slice_with_first_equals_the_range_of_the_whole(bits, small):
    (w, a, e), _ = small
    whole, res, _, _ = _encode(w, a, e, bits, "stochastic", 5, 6)
    cw = N * bits // 32
    for lo, hi in ((0, 512), (512, 1536), (1984, 2048)):
        part, pres, _, _ = _encode(w[lo:hi], a[lo:hi], e[lo:hi], bits, "stochastic", 5, 6, first=lo // 64)
        k = (hi - lo) * bits // 32
        assert torch.equal(part[:k], whole[lo * bits // 32:hi * bits // 32])
        assert torch.equal(part[k:], whole[cw + lo // 64:cw + hi // 64])
        assert torch.equal(_i32(pres), _i32(res[lo:hi]))
    other, _, _, _ = _encode(w[512:1536], a[512:1536], e[512:1536], bits, "stochastic", 5, 6, first=0)
    k = 1024 * bits // 32
    assert not torch.equal(other[:k], whole[512 * bits // 32:512 * bits // 32 + k])   # (another part of the stream)
    # far into the stream: the 64-bit float4 index carries into the counter's second word
    far, _, _, _ = _encode(w, a, e, bits, "stochastic", 5, 6, first=(1 << 28) - 8)
    want, _ = cp.torch_quantize_(w.cpu(), a.cpu(), e.cpu(), bits, "stochastic", SEED, 5, 6, first=(1 << 28) - 8)
    assert torch.equal(far.cpu(), want)


@pytest.mark.parametrize("bits", [8, 4])
def test_nothing_outside_the_buffers_is_written(bits, small):
    """Every buffer sits between 64-element canaries; payload, partial and stats start as garbage and
    every entry is overwritten; w and the anchor are not written."""
    C = 64
    (w0, a0, e0), _ = small
    words, grid = K.quant_words(N, bits), K.quant_grid(N)

    def framed(k, val, dt=torch.float32):
        big = torch.full((k + 2 * C,), val, dtype=dt, device=DEV)
        return big, big[C:C + k]

    wbig, w = framed(N, 1234.5)
    abig, a = framed(N, 99.0)
    ebig, e = framed(N, -3.0)
    pbig, p = framed(words, 0x5A5A5A5A, torch.int32)
    qbig, part = framed(3 * grid, -77.0, torch.float64)
    tbig, st = framed(4, -5.0, torch.float64)
    obig, out = framed(N, 55.0)
    sbig, sh = framed(N, 7.0, torch.bfloat16)
    w.copy_(w0)
    a.copy_(a0)
    e.copy_(e0)
    K.quant_encode(w, a, e, p, part, st, bits, True, SEED, 1, 2, 0)
    K.quant_decode_mean([p, p.clone()], a, out, sh, bits)
    torch.cuda.synchronize()
    for big, k, val in ((wbig, N, 1234.5), (abig, N, 99.0), (ebig, N, -3.0), (pbig, words, 0x5A5A5A5A),
                        (qbig, 3 * grid, -77.0), (tbig, 4, -5.0), (obig, N, 55.0), (sbig, N, 7.0)):
        for can in (big[:C], big[C + k:]):
            assert torch.equal(can, torch.full_like(can, val))
    assert torch.equal(w, w0) and torch.equal(a, a0)
    assert bool((part >= 0).all()) and float(st[0]) > 0 and float(st[3]) == 0.0     # (no entry keeps its garbage)
    want_e = e0.cpu().clone()
    want, _ = cp.torch_quantize_(w0.cpu(), a0.cpu(), want_e, bits, "stochastic", SEED, 1, 2)
    assert torch.equal(p.cpu(), want) and torch.equal(_i32(e.cpu()), _i32(want_e))
    assert torch.equal(sh.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)) and bool(torch.isfinite(out).all())


def test_run_to_run_determinism(wrap):
    (w, a, e), _ = wrap
    for bits in (8, 4):
        first = _encode(w, a, e, bits, "stochastic", 2, 3)
        again = _encode(w, a, e, bits, "stochastic", 2, 3)
        assert torch.equal(first[0], again[0]) and torch.equal(_i32(first[1]), _i32(again[1]))
        assert torch.equal(first[2].view(torch.int64), again[2].view(torch.int64))
        assert torch.equal(first[3].view(torch.int64), again[3].view(torch.int64))
        outs = []
        for _ in range(2):
            out = torch.empty(N_WRAP, device=DEV)
            K.quant_decode_mean([first[0], again[0], first[0]], a, out, None, bits)
            outs.append(out)
        assert torch.equal(_i32(outs[0]), _i32(outs[1]))


def _batch(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(S // 3, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = ids * mask
    ids[:, 0] = 101
    labels = torch.randint(0, 2, (B,), generator=g)
    return ids.cuda(), mask.cuda(), labels.cuda(), int(lens.sum())


def test_compressor_on_a_model_arena():
    """``Compressor`` on the default DistilBERT arena: two clients encode over two rounds (the second
    with a residual), the decoded mean is within the quantization step of the true mean, the pads stay
    +0, the shadow the kernel wrote is the shadow a refresh would write, and a graphed training step
    runs on the result."""
    model = DDoSClassifier(device=DEV, impl="hip", seed=3)
    A = model.arena
    n = A.numel
    assert n % 64 == 0
    live = torch.zeros(n, dtype=torch.bool, device=DEV)
    for name in A.names():
        off, shape = A.offsets[name]
        live[off:off + math.prod(shape)] = True
    assert int((~live).sum()) == n - A.n_params > 0
    c = cp.Compressor(8, rounding="stochastic", seed=SEED)
    g = torch.Generator(device=DEV).manual_seed(5)
    for r in range(2):
        anchor = A.master.clone()
        trained = [anchor + 1e-4 * (k + 1) * torch.randn(n, device=DEV, generator=g) * live for k in range(2)]
        ps = []
        for k in range(2):
            ps.append(c.encode_(trained[k], anchor, k, r))
            rep = c.last
            v = (trained[k] - anchor).double().norm() if r == 0 else None
            assert rep["payload_bytes"] == 4 * K.quant_words(n, 8) and abs(rep["ratio"] - cp.payload_ratio(8)) < 1e-9
            assert rep["bad_groups"] == 0 and 0 < rep["error_l2"] < 0.02 * rep["update_l2"]
            if v is not None:
                assert abs(rep["update_l2"] - float(v)) <= 2.0 ** -22 * float(v)
            assert abs(float(c.residuals[k].double().norm()) - rep["error_l2"]) <= 2.0 ** -22 * rep["error_l2"]
        c.decode_mean_(model, ps, anchor)
        torch.cuda.synchronize()
        mean = anchor.double() + 0.5 * ((trained[0] - anchor).double() + (trained[1] - anchor).double())
        # per element each client's error is below its group's scale (+ its carried residual)
        step = max(float(cp.split_payload(p.cpu(), n, 8)[1].max()) for p in ps)
        assert float((A.master.double() - mean).abs().max()) <= 2 * step + 1e-6
        assert not A.master[~live].view(torch.int32).any() and not A.shadow[~live].view(torch.int16).any()
        assert torch.equal(A.shadow.view(torch.int16), A.master.to(torch.bfloat16).view(torch.int16))
        assert all(not e[~live].view(torch.int32).any() for e in c.residuals.values())
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
    w8, w4, grid = K.quant_words(n, 8), K.quant_words(n, 4), K.quant_grid(n)
    w, a, e, out, sh = mk(), mk(), mk(), mk(), mk(dt=torch.bfloat16)
    p8, p4 = mk(w8, torch.int32), mk(w4, torch.int32)
    part, st = mk(3 * grid, torch.float64), mk(4, torch.float64)
    ext = K.ext()
    ok_enc = dict(w=w, anchor=a, residual=e, payload=p8, partial=part, stats=st, bits=8, stochastic=True, seed_lo=1,
                  seed_hi=2, round=3, client=4, first=0)
    ok_dec = dict(payloads=[p8, p8.clone()], anchor=a, out=out, shadow=sh, bits=8)

    def bad(fn, ok, **kw):
        with pytest.raises(RuntimeError):
            getattr(ext, fn)(**dict(ok, **kw))

    big = mk(2 * n)
    bad("quant_encode", ok_enc, w=mk(n - 4), anchor=mk(n - 4), residual=None)             # length: n % 64
    bad("quant_encode", ok_enc, w=mk(0), anchor=mk(0), residual=None, payload=mk(0, torch.int32))
    bad("quant_encode", ok_enc, anchor=mk(n - 64))
    bad("quant_encode", ok_enc, residual=mk(n + 64))
    bad("quant_encode", ok_enc, w=mk(dt=torch.float64))                                   # dtype
    bad("quant_encode", ok_enc, anchor=mk(dt=torch.bfloat16))
    bad("quant_encode", ok_enc, residual=mk(dt=torch.float16))
    bad("quant_encode", ok_enc, payload=mk(w8, torch.float32))
    bad("quant_encode", ok_enc, payload=mk(w8, torch.int64))
    bad("quant_encode", ok_enc, partial=mk(3 * grid, torch.float32))
    bad("quant_encode", ok_enc, stats=mk(4, torch.float32))
    bad("quant_encode", ok_enc, w=mk(2 * n)[::2])                                         # not contiguous
    bad("quant_encode", ok_enc, anchor=a.cpu())                                           # device
    bad("quant_encode", ok_enc, payload=p8.cpu())
    bad("quant_encode", ok_enc, stats=st.cpu())
    bad("quant_encode", ok_enc, anchor=w)                                                 # overlap
    bad("quant_encode", ok_enc, residual=w)
    bad("quant_encode", ok_enc, residual=a)
    bad("quant_encode", ok_enc, w=big[:n], anchor=big[n // 2:n // 2 + n])
    bad("quant_encode", ok_enc, w=big[:n], payload=big[n // 2:n // 2 + w8].view(torch.int32))
    bad("quant_encode", ok_enc, payload=mk(w8 - 1, torch.int32))                          # short payload
    bad("quant_encode", ok_enc, payload=p4)
    bad("quant_encode", ok_enc, bits=4)                                                   # (an int8 payload at int4)
    bad("quant_encode", ok_enc, partial=mk(3 * grid - 1, torch.float64))
    bad("quant_encode", ok_enc, stats=mk(3, torch.float64))
    for bits in (0, 2, 16, 32, -8):                                                       # bits
        bad("quant_encode", ok_enc, bits=bits)
        bad("quant_decode_mean", ok_dec, bits=bits)
    for kw in (dict(round=-1), dict(client=-1), dict(first=-1), dict(round=1 << 32), dict(client=1 << 32),
               dict(seed_lo=-1), dict(seed_hi=1 << 32), dict(first=(1 << 63) // 16)):
        bad("quant_encode", ok_enc, **kw)
    bad("quant_decode_mean", ok_dec, payloads=[])                                         # M
    bad("quant_decode_mean", ok_dec, payloads=[p8] * 17)
    bad("quant_decode_mean", ok_dec, payloads=[p8, mk(w8 - 1, torch.int32)])              # short payload
    bad("quant_decode_mean", ok_dec, payloads=[p4])
    bad("quant_decode_mean", ok_dec, payloads=[p8], bits=4)
    bad("quant_decode_mean", ok_dec, payloads=[p8.float()])                               # dtype
    bad("quant_decode_mean", ok_dec, out=mk(dt=torch.float64))
    bad("quant_decode_mean", ok_dec, shadow=mk())
    bad("quant_decode_mean", ok_dec, anchor=mk(n - 64))                                   # length
    bad("quant_decode_mean", ok_dec, shadow=mk(n - 64, torch.bfloat16))
    bad("quant_decode_mean", ok_dec, out=mk(n - 4), anchor=mk(n - 4), shadow=None)
    bad("quant_decode_mean", ok_dec, payloads=[p8.cpu()])                                 # device
    bad("quant_decode_mean", ok_dec, anchor=a.cpu())
    bad("quant_decode_mean", ok_dec, out=a)                                               # overlap
    bad("quant_decode_mean", ok_dec, out=big[:n], anchor=big[n // 2:n // 2 + n])
    bad("quant_decode_mean", ok_dec, out=big[:n], payloads=[big[n // 2:n // 2 + w8].view(torch.int32)])
    bad("quant_decode_mean", ok_dec, out=big[:n], shadow=big[n // 2:n].view(torch.bfloat16))
    bad("quant_decode_mean", ok_dec, anchor=big[:n], shadow=big[n // 2:n].view(torch.bfloat16))
    for args in ((100, 8), (128, 3), (0, 8)):
        with pytest.raises(RuntimeError):
            K.quant_words(*args)
    with pytest.raises(ValueError):
        K.quant_encode(w, a, e, p8, part, st, 8, True, 1 << 64, 0, 0)
    torch.cuda.synchronize()
    assert all(torch.equal(t, torch.ones_like(t)) for t in (w, a, e, out, sh, p8, p4, part, st, big))
    K.quant_encode(big[:n], big[n:], None, p8, part, st, 8, False, SEED, 0, 0)            # beside w: accepted
    K.quant_decode_mean([p8], big[n:], out, sh, 8)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0, 0.0, 0.0, 0.0] and not p8.any() and torch.equal(big, torch.ones_like(big))
    assert torch.equal(out, torch.ones_like(out))
