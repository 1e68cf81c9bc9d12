"""The top-k sparsification kernels on the GPU (csrc/kernels/sparsify.hip through ``ops.kernels.topk_*``
and ``parallel.compress.TopKCompressor``): encode bit for bit against the torch specification (payload,
residual, sent) at three lengths -- two chunks and a ragged one, the smallest, and one where every
chunk loop wraps with a ragged tail -- crafted inputs for each radix level, the stats against fp64
within a derived bound, decode_mean bit for bit, the decoder's guards between canaries, canaries around
every buffer, run-to-run determinism, a real model arena, and the binding's refusals.

The specification runs on the CPU; no input relies on denormals."""
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
CH = 4096
GRID_CAP = 1024
N = 2 * CH + 3 * 64                        # two chunks and a ragged one
N_MIN = 64                                 # one ragged chunk
N_WRAP = (GRID_CAP + 3) * CH + 5 * 64      # just above the block cap: every chunk loop wraps, ragged tail
STATS = 8


def _make(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    anchor = 0.05 * torch.randn(n, device=DEV, generator=g)
    w = anchor + 1e-3 * torch.randn(n, device=DEV, generator=g) * torch.rand(n, device=DEV, generator=g)
    e = 1e-5 * torch.randn(n, device=DEV, generator=g)
    if n > 1024:                           # rows no step touched: the update is exactly zero
        w[n // 3:n // 3 + 700] = anchor[n // 3:n // 3 + 700]
        e[n // 3:n // 3 + 700] = 0.0
    if n > 128:
        for p in (0, n - 64):              # 64-float alignment pads: +0 in w, anchor and residual
            w[p:p + 64] = 0.0
            anchor[p:p + 64] = 0.0
            e[p:p + 64] = 0.0
    return w, anchor, e


@pytest.fixture(scope="module")
def inputs():
    """{n: ((w, anchor, residual) on the device, the same on the host)}; computed once, never written."""
    out = {}
    for n, seed in ((N, 17), (N_MIN, 19), (N_WRAP, 23)):
        t = _make(n, seed)
        out[n] = (t, tuple(x.cpu() for x in t))
    return out


def _i32(t):
    return t.view(torch.int32)


def _work_parts(work, n):
    """(state int32 [16], partial float64 [grid][2]) inside ``work`` (sparsify.hip tk_carve)."""
    C, grid = (n + CH - 1) // CH, K.topk_grid(n)
    lo = n * 4 + (2048 + 1024 + 1024) * 4
    state = work[lo:lo + 64].view(torch.int32)
    plo = lo + 64 + C * 16
    return state, work[plo:plo + grid * 16].view(torch.float64).view(-1, 2)


def _encode(w, a, e, k):
    n = w.numel()
    payload = torch.full((K.topk_words(n, k),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    work = torch.full((K.topk_work_bytes(n),), 0xA5, dtype=torch.uint8, device=DEV)
    stats = torch.full((STATS,), -7.0, dtype=torch.float64, device=DEV)
    res = None if e is None else e.clone()
    K.topk_encode(w, a, res, payload, work, stats, k)
    return payload, res, stats, work


def _check(w, a, e, k, wc=None, ac=None, ec=None):
    """Encode on the device and by the specification: payload, residual, sent, bad and threshold equal."""
    wc = w.cpu() if wc is None else wc
    ac = a.cpu() if ac is None else ac
    want_e = None if e is None else (e.cpu() if ec is None else ec).clone()
    payload, res, stats, _ = _encode(w, a, e, k)
    want, rep = cp.torch_topk_encode_(wc, ac, want_e, k)
    assert torch.equal(payload.cpu(), want)
    if e is not None:
        assert torch.equal(_i32(res.cpu()), _i32(want_e))
    up, er, bad, sent, thr, z0, z1, z2 = stats.tolist()
    assert (bad, sent, thr) == (float(rep["bad_elems"]), float(rep["sent"]), rep["threshold"])
    assert z0 == z1 == z2 == 0.0
    for got, ref in ((up, rep["update_l2"]), (er, rep["error_l2"])):   # (3e38 squared three times: inf in fp32)
        assert got == ref or abs(got - ref) <= 2.0 ** -23 * ref
    return payload, res, rep


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("n", [N, N_MIN, N_WRAP])
def test_encode_equals_the_specification(n, feedback, inputs):
    (w, a, e), (wc, ac, ec) = inputs[n]
    C = (n + CH - 1) // CH
    assert K.topk_grid(n) == min(C, GRID_CAP) and K.topk_work_bytes(n) >= 4 * n
    for k in sorted({cp.topk_k(n, 0.01), 1, n // 2}):
        assert K.topk_words(n, k) == cp.topk_words(n, k)
        payload, res, rep = _check(w, a, e if feedback else None, k, wc, ac, ec)
        assert rep["sent"] == k and rep["bad_elems"] == 0
        if n > 128 and feedback:
            assert not _i32(res[:64]).any() and not _i32(res[-64:]).any()      # pads: residual +0


def _bits_tensor(bits):
    return bits.to(torch.int32).view(torch.float32)


def _crafted():
    """(name, w, ks): anchor 0; each case bears on one part of the select."""
    i = torch.arange(N, dtype=torch.int64)
    g = torch.Generator().manual_seed(11)
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    cases = []
    # level 0 alone decides: keys differ only in the top 11 bits (exponent and three mantissa bits)
    top = _bits_tensor((((i * 7) % 40 + 100) << 23) | (((i * 5) % 8) << 20))
    cases.append(("top bits", top * sign, (1, 9, 500, N // 2)))
    # level 1 alone: one top bin, bits 19 .. 10 vary
    cases.append(("middle bits", _bits_tensor(0x3F800000 | (((i * 37) % 1024) << 10)) * sign, (1, 9, 500, N // 2)))
    # level 2 alone: only the lowest mantissa bit differs
    cases.append(("lowest bit", _bits_tensor(0x3F800000 | ((i * 3 + i // 7) % 2)) * sign, (1, 9, 500, N // 2)))
    cases.append(("low ten bits", _bits_tensor(0x3F800000 | ((i * 131) % 1024)) * sign, (3, 500, N // 2)))
    cases.append(("all equal", torch.full((N,), -0.75), (1, 100, CH + 1, N // 2)))
    cases.append(("all zero", torch.zeros(N), (1, 100, N // 2)))
    mixed = 1e-3 * torch.randn(N, generator=g)
    mixed[[5, CH - 1, CH, N - 1]] = torch.tensor([3e38, -3e38, 3e38, 3e38])
    mixed[6::2] = 1e-30
    cases.append(("3e38 next to 1e-30", mixed, (2, 4, 5, 100, N // 2)))
    cases.append(("negative", -torch.rand(N, generator=g) - 0.5, (1, 77, N // 2)))
    ties = 1e-3 * torch.randn(N, generator=g)
    ties[[CH - 3, CH - 1, CH, CH + 2, 2 * CH - 1, 2 * CH + 5]] = torch.tensor([0.25, -0.25, 0.25, -0.25, 0.25, 0.25])
    ties[[7, CH + 9, 2 * CH + 100]] = torch.tensor([1.0, -2.0, 3.0])
    cases.append(("ties across a chunk boundary", ties, (4, 5, 6, 7, 8, 9, 10)))
    few = torch.zeros(N)
    few[[50, CH + 1, N - 2]] = torch.tensor([-2.0, 1.0, -0.0])
    cases.append(("fewer nonzero than k", few, (2, 3, 10, N // 2)))
    bad = 1e-3 * torch.randn(N, generator=g)
    bad[[0, 63, CH - 1, CH, N - 1]] = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan"), float("inf")])
    bad[100:164] = float("nan")
    cases.append(("NaN and inf", bad, (1, 100, N // 2)))
    return cases


@pytest.mark.parametrize("case", _crafted(), ids=lambda c: c[0])
def test_crafted_inputs(case):
    name, wc, ks = case
    zero = torch.zeros(N)
    w, a = wc.to(DEV), zero.to(DEV)
    for k in ks:
        _check(w, a, a.clone(), k, wc, zero, zero)
        payload, _, rep = _check(w, a, None, k, wc, zero, None)
    if name == "NaN and inf":
        assert rep["bad_elems"] == 69 and math.isfinite(rep["update_l2"])
    if name == "3e38 next to 1e-30":
        assert rep["update_l2"] == float("inf") and rep["sent"] == N // 2
    if name == "all equal":
        off = cp.split_topk_payload(payload.cpu(), N, N // 2)[0]
        assert off.tolist() == [0, CH, N // 2, N // 2]                      # the lowest indices


def test_fewer_candidates_than_k():
    """n = 64 with 60 NaNs and k = 8: the four candidates are sent, the rest of the payload is 0; and a
    tensor with no candidate at all sends nothing."""
    wc = torch.full((N_MIN,), float("nan"))
    wc[[3, 17, 40, 63]] = torch.tensor([1.0, 0.0, -3.0, 2.0])
    zero = torch.zeros(N_MIN)
    payload, res, rep = _check(wc.to(DEV), zero.to(DEV), zero.to(DEV), 8, wc, zero, zero)
    assert rep["sent"] == 4 and rep["bad_elems"] == 60 and rep["threshold"] == 0.0 and not _i32(res).any()
    off, val, loc = cp.split_topk_payload(payload.cpu(), N_MIN, 8)
    assert off.tolist() == [0, 4] and loc.tolist() == [3, 17, 40, 63, 0, 0, 0, 0]
    wc = torch.full((N_MIN,), float("inf"))
    payload, res, rep = _check(wc.to(DEV), zero.to(DEV), zero.to(DEV), 5, wc, zero, zero)
    assert rep["sent"] == 0 and rep["bad_elems"] == 64 and rep["threshold"] == 0.0 and not payload.any()


@pytest.mark.parametrize("n", [N, N_WRAP])
def test_stats(n, inputs):
    """|v| and |e'| against fp64.  The device squares in fp64 (exact for fp32 inputs) and adds n
    non-negative doubles in a fixed order; so does the reference, in another order: the two sums of
    squares agree within 2 n 2^-53, their roots within half that, and the fp32 roundings of two roots
    that close are at most one ulp apart.  bad_elems, sent and threshold are exact."""
    (w, a, e), _ = inputs[n]
    w = w.clone()
    bad = [200, n // 2 + 1, n - 70]
    for j, i in enumerate(bad):
        w[i] = float("nan") if j % 2 == 0 else float("inf")
    k = cp.topk_k(n, 0.01)
    payload, res, stats, work = _encode(w, a, e, k)
    good = torch.ones(n, dtype=torch.bool, device=DEV)
    good[bad] = False
    v = ((w - a) + e)[good].double()
    up, er, nb, sent, thr = stats.tolist()[:5]
    assert nb == float(len(bad)) and sent == float(k)
    mags = v.abs().float().sort(descending=True).values
    assert thr == float(mags[k - 1])
    state, p = _work_parts(work, n)
    assert bool(torch.isfinite(p).all()) and int(state[2]) == len(bad) and int(state[3]) == k
    assert not _i32(res[bad]).any()
    for got, S, ref in ((up, float(p[:, 0].sum()), v), (er, float(p[:, 1].sum()), res[good].double())):
        want = float(ref.square().sum())
        rel = abs(S - want) / want
        print(f"topk_encode n={n}: relative error of a sum of squares {rel:.3e} (bound {2 * n * 2.0 ** -53:.3e})")
        assert rel <= 2 * n * 2.0 ** -53
        r32 = torch.tensor(math.sqrt(want), dtype=torch.float64).to(torch.float32)
        ulp = abs(float(torch.nextafter(r32, torch.tensor(float("inf"))) - r32))
        assert abs(got - float(r32)) <= ulp and got == float(torch.tensor(got).float())


K_DEC = 50


@pytest.fixture(scope="module")
def payloads(inputs):
    """16 payloads at N with K_DEC entries each (CPU specification) that share most of their indices."""
    _, (_, ac, _) = inputs[N]
    hot = torch.randperm(N - 128, generator=torch.Generator().manual_seed(1))[:40] + 64
    ps = []
    for c in range(16):
        g = torch.Generator().manual_seed(100 + c)
        wk = ac + 1e-3 * torch.randn(N, generator=g)
        wk[hot] += 0.01 * (c + 1) * torch.randn(40, generator=g)
        wk[:64] = 0.0
        ps.append(cp.torch_topk_encode_(wk, ac, None, K_DEC)[0])
    return ps


@pytest.mark.parametrize("M", [1, 2, 3, 8, 16])
def test_decode_mean_equals_the_specification(M, inputs, payloads):
    (_, a, _), (_, ac, _) = inputs[N]
    ps = payloads[:M]
    for shadow in (True, False):
        out = torch.full((N,), 7.0, device=DEV)
        sh = torch.full((N,), 7.0, dtype=torch.bfloat16, device=DEV) if shadow else None
        K.topk_decode_mean([p.to(DEV) for p in ps], a, out, sh, K_DEC)
        want, wsh = torch.empty(N), torch.empty(N, dtype=torch.bfloat16)
        cp.torch_topk_decode_mean_(ps, ac, want, wsh, K_DEC)
        assert torch.equal(_i32(out.cpu()), _i32(want))
        if shadow:
            assert torch.equal(sh.cpu().view(torch.int16), wsh.view(torch.int16))
        assert not _i32(out[:64]).any()                           # the pad stays +0
    if M >= 2:                                                    # the order of the payloads is the order of the sum
        out2 = torch.empty(N, device=DEV)
        K.topk_decode_mean([p.to(DEV) for p in reversed(ps)], a, out2, None, K_DEC)
        want2 = torch.empty(N)
        cp.torch_topk_decode_mean_(list(reversed(ps)), ac, want2, None, K_DEC)
        assert torch.equal(_i32(out2.cpu()), _i32(want2))


def test_decode_mean_adds_in_payload_order():
    """1e8, -1e8 and 1 on one index: (1e8 - 1e8) + 1 = 1, (1e8 + 1) - 1e8 = 0."""
    zero = torch.zeros(N)
    one = []
    for x in (1e8, -1e8, 1.0):
        w = zero.clone()
        w[CH + 77] = x
        one.append(cp.torch_topk_encode_(w, zero, None, 1)[0])
    for order, expect in (((0, 1, 2), float(torch.tensor(1.0) * torch.tensor(1.0 / 3))), ((0, 2, 1), 0.0)):
        ps = [one[j] for j in order]
        out = torch.empty(N, device=DEV)
        K.topk_decode_mean([p.to(DEV) for p in ps], zero.to(DEV), out, None, 1)
        want = torch.empty(N)
        cp.torch_topk_decode_mean_(ps, zero, want, None, 1)
        assert torch.equal(_i32(out.cpu()), _i32(want)) and float(out[CH + 77]) == expect


def test_decode_mean_wrap(inputs):
    """decode_mean where the chunk loop wraps, M = 2: round trip of two encodes."""
    (w, a, e), (_, ac, _) = inputs[N_WRAP]
    k = cp.topk_k(N_WRAP, 0.01)
    p0 = _encode(w, a, e, k)[0]
    p1 = _encode(w, a, None, k)[0]
    out = torch.empty(N_WRAP, device=DEV)
    sh = torch.empty(N_WRAP, dtype=torch.bfloat16, device=DEV)
    K.topk_decode_mean([p0, p1], a, out, sh, k)
    want, wsh = torch.empty(N_WRAP), torch.empty(N_WRAP, dtype=torch.bfloat16)
    cp.torch_topk_decode_mean_([p0.cpu(), p1.cpu()], ac, want, wsh, k)
    assert torch.equal(_i32(out.cpu()), _i32(want)) and torch.equal(sh.cpu().view(torch.int16), wsh.view(torch.int16))


def _framed(k, val, dt=torch.float32, C=CH):
    big = torch.full((k + 2 * C,), val, dtype=dt, device=DEV)
    return big, big[C:C + k]


def _intact(big, k, val, C=CH):
    return all(torch.equal(can, torch.full_like(can, val)) for can in (big[:C], big[C + k:]))


def test_decode_guards(inputs):
    """Payloads with a descending offset, offsets above k and below 0 (off by at most 8 entries) and a
    local index beyond the ragged chunk (below 4096) decode like the specification, which clamps and
    drops; every tensor is a window of a larger allocation whose margins (4096 floats; 64 words for a
    payload) stay as they were."""
    (_, a0, _), (_, ac, _) = inputs[N]
    C = 3
    # hand-made payloads: offsets [0, 20, 40, 50], entry j at local index 3 j + 1 -- all distinct and inside
    # the ragged chunk's 192 elements, so whichever entries a chunk reads, it reads no index twice
    local = 3 * torch.arange(K_DEC, dtype=torch.int64) + 1
    crafted = []
    for edit in (lambda p: (p.__setitem__(1, 24), p.__setitem__(2, 18)),                # descending
                 lambda p: p.__setitem__(3, K_DEC + 8),                                 # above k
                 lambda p: (p.__setitem__(0, K_DEC + 3), p.__setitem__(1, K_DEC + 5)),  # first above k
                 lambda p: p.__setitem__(1, -4),                                        # negative
                 lambda p: p.__setitem__(C + 1 + K_DEC + 24, 300 | (4095 << 16))):      # beyond the ragged chunk
        g = torch.Generator().manual_seed(40 + len(crafted))
        p = torch.zeros(cp.topk_words(N, K_DEC), dtype=torch.int32)
        p[:C + 1] = torch.tensor([0, 20, 40, K_DEC], dtype=torch.int32)
        p[C + 1:C + 1 + K_DEC] = (0.01 * torch.randn(K_DEC, generator=g)).view(torch.int32)
        p[C + 1 + K_DEC:] = (local[0::2] | (local[1::2] << 16)).to(torch.int32)
        edit(p)
        crafted.append(p)
    words = cp.topk_words(N, K_DEC)
    abig, a = _framed(N, 99.0)
    obig, out = _framed(N, 55.0)
    sbig, sh = _framed(N, 7.0, torch.bfloat16)
    a.copy_(a0)
    frames = [_framed(words, 0, torch.int32, 64) for _ in crafted]
    for (_, win), p in zip(frames, crafted):
        win.copy_(p)
    for M in (1, len(crafted)):
        K.topk_decode_mean([win for _, win in frames[:M]], a, out, sh, K_DEC)
        torch.cuda.synchronize()
        want, wsh = torch.empty(N), torch.empty(N, dtype=torch.bfloat16)
        cp.torch_topk_decode_mean_(crafted[:M], ac, want, wsh, K_DEC)
        assert torch.equal(_i32(out.cpu()), _i32(want)) and torch.equal(sh.cpu().view(torch.int16), wsh.view(torch.int16))
    for j in range(len(crafted)):                             # each alone, too
        K.topk_decode_mean([frames[j][1]], a, out, None, K_DEC)
        want = torch.empty(N)
        cp.torch_topk_decode_mean_([crafted[j]], ac, want, None, K_DEC)
        assert torch.equal(_i32(out.cpu()), _i32(want)), j
    assert _intact(abig, N, 99.0) and _intact(obig, N, 55.0) and _intact(sbig, N, 7.0)
    assert all(_intact(big, words, 0, 64) for big, _ in frames)
    assert all(torch.equal(win.cpu(), p) for (_, win), p in zip(frames, crafted))


@pytest.mark.parametrize("feedback", [True, False])
def test_nothing_outside_the_buffers_is_written(feedback, inputs):
    """Every buffer sits between canaries of 4096 elements; payload, work and stats start as garbage and
    every payload and stats word is overwritten; w and the anchor are not written."""
    (w0, a0, e0), (wc, ac, ec) = inputs[N]
    k = 90
    words, wbytes = K.topk_words(N, k), K.topk_work_bytes(N)
    wbig, w = _framed(N, 1234.5)
    abig, a = _framed(N, 99.0)
    ebig, e = _framed(N, -3.0)
    pbig, p = _framed(words, 0x5A5A5A5A, torch.int32)
    kbig, work = _framed(wbytes, 0xA5, torch.uint8)
    tbig, st = _framed(STATS, -5.0, torch.float64)
    obig, out = _framed(N, 55.0)
    sbig, sh = _framed(N, 7.0, torch.bfloat16)
    w.copy_(w0)
    a.copy_(a0)
    e.copy_(e0)
    K.topk_encode(w, a, e if feedback else None, p, work, st, k)
    K.topk_decode_mean([p, p.clone()], a, out, sh, k)
    torch.cuda.synchronize()
    for big, cnt, val in ((wbig, N, 1234.5), (abig, N, 99.0), (ebig, N, -3.0), (pbig, words, 0x5A5A5A5A),
                          (kbig, wbytes, 0xA5), (tbig, STATS, -5.0), (obig, N, 55.0), (sbig, N, 7.0)):
        assert _intact(big, cnt, val)
    assert torch.equal(w, w0) and torch.equal(a, a0)
    want_e = ec.clone() if feedback else None
    want, rep = cp.torch_topk_encode_(wc, ac, want_e, k)
    assert torch.equal(p.cpu(), want)
    assert torch.equal(_i32(e.cpu()), _i32(want_e if feedback else ec))
    assert st.tolist()[2:] == [0.0, float(k), rep["threshold"], 0.0, 0.0, 0.0] and float(st[0]) > 0
    assert torch.equal(sh.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)) and bool(torch.isfinite(out).all())


def test_run_to_run_determinism(inputs):
    (w, a, e), _ = inputs[N_WRAP]
    k = cp.topk_k(N_WRAP, 0.01)
    first = _encode(w, a, e, k)
    again = _encode(w, a, e, k)
    assert torch.equal(first[0], again[0]) and torch.equal(_i32(first[1]), _i32(again[1]))
    assert torch.equal(first[2].view(torch.int64), again[2].view(torch.int64))
    for x, y in zip(_work_parts(first[3], N_WRAP), _work_parts(again[3], N_WRAP)):
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    outs = []
    for _ in range(2):
        out = torch.empty(N_WRAP, device=DEV)
        K.topk_decode_mean([first[0], again[0], first[0]], a, out, None, k)
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


def test_topk_compressor_on_a_model_arena():
    """``TopKCompressor`` on the default DistilBERT arena: two clients encode over two rounds (the second
    with a residual); what was sent plus the residual is the update bit for bit, everything above the
    threshold was sent, the decoded mean is the mean of the scattered payloads, the pads stay +0, the
    shadow the kernel wrote is the shadow a refresh would write, and a graphed training step runs on
    the result."""
    model = DDoSClassifier(device=DEV, impl="hip", seed=3)
    A = model.arena
    n = A.numel
    assert n % 64 == 0
    live = torch.zeros(n, dtype=torch.bool, device=DEV)
    for name in A.names():
        off, shape = A.offsets[name]
        live[off:off + math.prod(shape)] = True
    assert int((~live).sum()) == n - A.n_params > 0
    c = cp.TopKCompressor(0.01)
    k = c.k(n)
    assert k == n // 100 and c.words(n) == K.topk_words(n, k)
    g = torch.Generator(device=DEV).manual_seed(5)
    zero = torch.zeros(n, device=DEV)
    for r in range(2):
        anchor = A.master.clone()
        trained = [anchor + 1e-4 * (j + 1) * torch.randn(n, device=DEV, generator=g) * live for j in range(2)]
        ps, dense = [], []
        for j in range(2):
            before = c.residuals[j].clone() if j in c.residuals else zero
            v = (trained[j] - anchor) + before
            ps.append(c.encode_(trained[j], anchor, j, r))
            rep = c.last
            assert rep["payload_bytes"] == 4 * K.topk_words(n, k) and rep["ratio"] == n / K.topk_words(n, k) > 60
            assert rep["bad_elems"] == 0 and rep["sent"] == k and 0 < rep["error_l2"] < rep["update_l2"]
            d = torch.empty(n, device=DEV)
            K.topk_decode_mean([ps[-1]], zero, d, None, k)                   # 0 + val * 1: the sent entries
            dense.append(d)
            assert torch.equal(_i32(d + c.residuals[j]), _i32(v))
            assert int((d != 0).sum()) == k and float(d[d != 0].abs().min()) == rep["threshold"]
            assert int((v.abs() > rep["threshold"]).sum()) <= k and float(c.residuals[j].abs().max()) <= rep["threshold"]
            assert abs(rep["update_l2"] - float(v.double().norm())) <= 2.0 ** -22 * rep["update_l2"]
            assert abs(float(c.residuals[j].double().norm()) - rep["error_l2"]) <= 2.0 ** -22 * rep["error_l2"]
        c.decode_mean_(model, ps, anchor)
        torch.cuda.synchronize()
        assert torch.equal(_i32(A.master), _i32(anchor + (dense[0] + dense[1]) * 0.5))
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
    n, k = 2 * CH, 40
    mk = lambda cnt=n, dt=torch.float32: torch.ones(cnt, dtype=dt, device=DEV)  # noqa: E731
    words, wbytes = K.topk_words(n, k), K.topk_work_bytes(n)
    w, a, e, out, sh = mk(), mk(), mk(), mk(), mk(dt=torch.bfloat16)
    p = mk(words, torch.int32)
    work, st = mk(wbytes, torch.uint8), mk(STATS, torch.float64)
    ext = K.ext()
    ok_enc = dict(w=w, anchor=a, residual=e, payload=p, work=work, stats=st, k=k)
    ok_dec = dict(payloads=[p, p.clone()], anchor=a, out=out, shadow=sh, k=k)

    def bad(fn, ok, **kw):
        with pytest.raises(RuntimeError):
            getattr(ext, fn)(**dict(ok, **kw))

    big = mk(3 * n)
    bad("topk_encode", ok_enc, w=mk(n - 4), anchor=mk(n - 4), residual=None)              # length: n % 64
    bad("topk_encode", ok_enc, w=mk(0), anchor=mk(0), residual=None, payload=mk(0, torch.int32))
    bad("topk_encode", ok_enc, anchor=mk(n - 64))
    bad("topk_encode", ok_enc, residual=mk(n + 64))
    bad("topk_encode", ok_enc, w=mk(dt=torch.float64))                                    # dtype
    bad("topk_encode", ok_enc, anchor=mk(dt=torch.bfloat16))
    bad("topk_encode", ok_enc, residual=mk(dt=torch.float16))
    bad("topk_encode", ok_enc, payload=mk(words, torch.float32))
    bad("topk_encode", ok_enc, payload=mk(words, torch.int64))
    bad("topk_encode", ok_enc, work=mk(wbytes, torch.int8))
    bad("topk_encode", ok_enc, work=mk(wbytes // 4 + 4, torch.float32))
    bad("topk_encode", ok_enc, stats=mk(STATS, torch.float32))
    bad("topk_encode", ok_enc, w=mk(2 * n)[::2])                                          # not contiguous
    bad("topk_encode", ok_enc, anchor=a.cpu())                                            # device
    bad("topk_encode", ok_enc, payload=p.cpu())
    bad("topk_encode", ok_enc, work=work.cpu())
    bad("topk_encode", ok_enc, stats=st.cpu())
    bad("topk_encode", ok_enc, anchor=w)                                                  # overlap
    bad("topk_encode", ok_enc, residual=w)
    bad("topk_encode", ok_enc, residual=a)
    bad("topk_encode", ok_enc, w=big[:n], anchor=big[n // 2:n // 2 + n])
    bad("topk_encode", ok_enc, w=big[:n], payload=big[n // 2:n // 2 + words].view(torch.int32))
    bad("topk_encode", ok_enc, w=big[:n], work=big[n // 2:n // 2 + wbytes // 4].view(torch.uint8))
    bad("topk_encode", ok_enc, payload=mk(words - 1, torch.int32))                        # extents
    bad("topk_encode", ok_enc, payload=mk(words + 1, torch.int32))
    bad("topk_encode", ok_enc, work=mk(wbytes - 1, torch.uint8))
    bad("topk_encode", ok_enc, work=mk(wbytes + 16, torch.uint8)[4:4 + wbytes])           # (not 16-byte aligned)
    bad("topk_encode", ok_enc, stats=mk(STATS - 1, torch.float64))
    bad("topk_encode", ok_enc, stats=mk(4, torch.float64))
    for kk in (0, -1, k + 1, n // 2 + 1, n, 1 << 40):                                     # k
        bad("topk_encode", ok_enc, k=kk)
        bad("topk_decode_mean", ok_dec, k=kk)
    bad("topk_decode_mean", ok_dec, payloads=[])                                          # M
    bad("topk_decode_mean", ok_dec, payloads=[p] * 17)
    bad("topk_decode_mean", ok_dec, payloads=[p, mk(words - 1, torch.int32)])             # short payload
    bad("topk_decode_mean", ok_dec, payloads=[p.float()])                                 # dtype
    bad("topk_decode_mean", ok_dec, out=mk(dt=torch.float64))
    bad("topk_decode_mean", ok_dec, shadow=mk())
    bad("topk_decode_mean", ok_dec, anchor=mk(n - 64))                                    # length
    bad("topk_decode_mean", ok_dec, shadow=mk(n - 64, torch.bfloat16))
    bad("topk_decode_mean", ok_dec, out=mk(n - 4), anchor=mk(n - 4), shadow=None)
    bad("topk_decode_mean", ok_dec, payloads=[p.cpu()])                                   # device
    bad("topk_decode_mean", ok_dec, anchor=a.cpu())
    bad("topk_decode_mean", ok_dec, out=a)                                                # overlap
    bad("topk_decode_mean", ok_dec, out=big[:n], anchor=big[n // 2:n // 2 + n])
    bad("topk_decode_mean", ok_dec, out=big[:n], payloads=[big[n // 2:n // 2 + words].view(torch.int32)])
    bad("topk_decode_mean", ok_dec, out=big[:n], shadow=big[n // 2:n].view(torch.bfloat16))
    bad("topk_decode_mean", ok_dec, anchor=big[:n], shadow=big[n // 2:n].view(torch.bfloat16))
    for args in ((100, 1), (128, 0), (128, 65), (0, 1), (1 << 31, 5)):
        with pytest.raises(RuntimeError):
            K.topk_words(*args)
    for nn in (100, 0, 1 << 31):
        with pytest.raises(RuntimeError):
            K.topk_work_bytes(nn)
    torch.cuda.synchronize()
    assert all(torch.equal(t, torch.ones_like(t)) for t in (w, a, e, out, sh, p, work, st, big))
    K.topk_encode(big[:n], big[n:2 * n], None, p, work, st, k)                            # beside w: accepted
    K.topk_decode_mean([p], big[n:2 * n], out, sh, k)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0, 0.0, 0.0, float(k), 0.0, 0.0, 0.0, 0.0] and torch.equal(big, torch.ones_like(big))
    off, val, loc = cp.split_topk_payload(p.cpu(), n, k)
    assert off.tolist() == [0, k, k] and not _i32(val).any() and loc.tolist() == list(range(k))
    assert torch.equal(out, torch.ones_like(out))
