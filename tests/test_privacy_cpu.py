"""Client-level differential privacy on the CPU (parallel/privacy.py: clip + Gaussian noise, DP-FedAvg):
the Philox4x32-10 known answers, the statistics of the Gaussian stream, the torch specification against
a hand-written loop, the accountant, the configuration plumbing and its refusals, the untouched default
path, the virtual run against the 2-rank gloo run bit for bit, a clip-only run, and the composition
with a robust aggregator and a server optimizer."""
import argparse
import math
import os
import socket
import struct
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"

from importlib import import_module  # noqa: E402

config = import_module(f"{PKG}.config")
data_pkg = import_module(f"{PKG}.data")
models = import_module(f"{PKG}.models")
runner = import_module(f"{PKG}.fed.runner")
pv = import_module(f"{PKG}.parallel.privacy")

SEED = 0x5EEDF00DCAFE
N_DRAWS = 1 << 22
PRIVACY_KEYS = ("update_l2", "clipped", "privacy_sigma", "privacy_epsilon")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _clear_rank_env():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)


def _single_thread(fn):
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)  # (CPU GEMM reductions split by thread count: same count on both sides)
    try:
        return fn()
    finally:
        torch.set_num_threads(nthreads)


# ------------------------------------------------------------------ the generator
def test_philox_known_answers():
    """Random123's known-answer tests of philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in pv.philox4x32_10(ctr, key)) == want
    # batched: one key for all counters, and one key per counter
    got = pv.philox4x32_10([k[0] for k in kat], [k[1] for k in kat])
    assert [tuple(int(x) for x in row) for row in got] == [k[2] for k in kat]
    got = pv.philox4x32_10([kat[0][0], kat[0][0]], kat[0][1])
    assert [tuple(int(x) for x in row) for row in got] == [kat[0][2]] * 2


@pytest.fixture(scope="module")
def streams():
    """2^22 draws of three streams of one seed; computed once, never written."""
    return {rc: pv.torch_gauss(N_DRAWS, SEED, *rc).double() for rc in ((0, 0), (1, 0), (0, 1))}


def gauss_statistics(streams):
    """5-sigma bounds (mean, variance, kurtosis, lag-1 and cross-stream correlation; max |g| <= 5.77)
    on three [N] fp64 streams keyed (0, 0), (1, 0), (0, 1); returns the figures in units of sigma
    (tests/test_privacy_gpu.py repeats it on the device's output)."""
    figs = {}
    for rc, g in streams.items():
        N = g.numel()
        mean, var = float(g.mean()), float(g.var(unbiased=False))
        kurt = float(((g - mean) ** 4).mean()) / var ** 2
        lag1 = float((g[:-1] * g[1:]).mean())
        figs[rc] = (abs(mean) * math.sqrt(N), abs(var - 1.0) / math.sqrt(2.0 / N),
                    abs(kurt - 3.0) / math.sqrt(24.0 / N), abs(lag1) * math.sqrt(N - 1), float(g.abs().max()))
        assert abs(mean) <= 5.0 / math.sqrt(N), (rc, mean)
        assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N), (rc, var)
        assert abs(kurt - 3.0) <= 5.0 * math.sqrt(24.0 / N), (rc, kurt)
        assert abs(lag1) <= 5.0 / math.sqrt(N - 1), (rc, lag1)
        assert float(g.abs().max()) <= 5.77, rc
    keys = list(streams)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            a, b = streams[keys[i]], streams[keys[j]]
            cross = float((a * b).mean())
            figs[(keys[i], keys[j])] = abs(cross) * math.sqrt(a.numel())
            assert abs(cross) <= 5.0 / math.sqrt(a.numel()), (keys[i], keys[j], cross)
    return figs


def test_gauss_statistics(streams):
    figs = gauss_statistics(streams)
    print("gauss statistics (units of sigma; max |g| last):", figs)


def test_gauss_indexing_and_streams():
    """A value depends on its global index alone; round, client and seed each select another stream;
    the counter's second word takes over past 2^32 float4."""
    full = pv.torch_gauss(4096, SEED, 3, 5)
    assert torch.equal(pv.torch_gauss(4096, SEED, 3, 5), full)
    assert torch.equal(pv.torch_gauss(1024, SEED, 3, 5, first4=100), full[400:1424])
    assert torch.equal(pv.torch_gauss(10, SEED, 3, 5), full[:10])          # (n need not be a multiple of 4)
    for other in (pv.torch_gauss(4096, SEED, 4, 5), pv.torch_gauss(4096, SEED, 3, 6),
                  pv.torch_gauss(4096, SEED + 1, 3, 5), pv.torch_gauss(4096, SEED + (1 << 32), 3, 5)):
        assert not torch.equal(other, full) and float((other == full).float().mean()) < 0.01
    hi = pv.torch_gauss(64, SEED, 0, 0, first4=(1 << 32) - 8)
    assert torch.equal(hi[32:], pv.torch_gauss(32, SEED, 0, 0, first4=1 << 32))
    assert not torch.equal(hi[32:], pv.torch_gauss(32, SEED, 0, 0, first4=0))
    # the first block by hand: counter (0, 0, round, client), key (seed lo, seed hi)
    x = [int(v) for v in pv.philox4x32_10((0, 0, 3, 5), (SEED & 0xFFFFFFFF, SEED >> 32))]
    u1, u2 = ((x[0] >> 8) + 1) * 2.0 ** -24, (x[1] >> 8) * 2.0 ** -24
    r = math.sqrt(-2.0 * math.log(u1))
    want = [r * math.cos(2 * math.pi * u2), r * math.sin(2 * math.pi * u2)]
    assert [float(full[0]), float(full[1])] == [float(np.float32(v)) for v in want]
    for bad in (dict(round=-1), dict(client=-1), dict(first4=-1), dict(round=1 << 32), dict(seed=-1), dict(seed=1 << 64)):
        kw = dict(dict(n=4, seed=SEED, round=0, client=0), **bad)
        with pytest.raises(ValueError):
            pv.torch_gauss(**kw)


# ------------------------------------------------------------------ the specification
def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _loop(w, a, clip, sigma, g):
    """The specification, element by element in Python floats rounded to fp32 after every operation."""
    n = len(w)
    d = [_f32(w[i] - a[i]) for i in range(n)]
    S = 0.0
    for x in d:
        S += x * x  # (fp64: a product of two fp32 values is exact in it)
    norm = np.float32(math.sqrt(S)) if math.isfinite(S) else np.float32(S)
    if not np.isfinite(norm):
        flag, scale, u = 2, 0.0, list(a)
    elif norm > np.float32(clip):
        flag, scale = 1, float(np.float32(clip) / norm)
        u = [_f32(a[i] + _f32(scale * d[i])) for i in range(n)]
    else:
        flag, scale, u = 0, 1.0, list(w)
    if sigma != 0.0:
        u = [_f32(u[i] + _f32(sigma * g[i])) for i in range(n)]
    return u, float(norm), scale, flag


def _vectors(n=64, seed=0, spread=1e-3):
    gen = torch.Generator().manual_seed(seed)
    a = 0.05 * torch.randn(n, generator=gen)
    w = a + spread * torch.randn(n, generator=gen)
    return w, a


def _bits(t):
    return t.view(torch.int32).tolist()


@pytest.mark.parametrize("sigma", [0.0, 0.0125])
def test_specification_against_a_loop(sigma):
    sigma = pv.f32(sigma)
    w, a = _vectors()
    norm = float((w - a).double().norm())
    g = pv.torch_gauss(64, SEED, 2, 1).tolist()
    for clip, flag in ((2.0 * norm, 0), (0.25 * norm, 1)):
        got = w.clone()
        rep = pv.torch_privatize_(got, a, clip, sigma, SEED, 2, 1)
        want, n_, scale, f_ = _loop(w.tolist(), a.tolist(), clip, sigma, g)
        assert f_ == flag == rep["clipped"] and rep["update_l2"] == n_ and rep["scale"] == scale
        assert rep["sigma"] == sigma
        assert _bits(got) == _bits(torch.tensor(want)), (clip, sigma)
        if flag == 0 and sigma == 0.0:
            assert _bits(got) == _bits(w)                      # identity, bit for bit
        if flag == 1 and sigma == 0.0:
            assert float((got - a).double().norm()) <= clip * (1 + 1e-6)
            assert float((got - a).double().norm()) >= clip * (1 - 1e-4)
    # the device's stats in place of the norm pass
    got = w.clone()
    rep = pv.torch_privatize_(got, a, 1.0, sigma, SEED, 2, 1, stats=torch.tensor([7.0, 0.5, 1.0, 0.0]))
    assert rep["update_l2"] == 7.0 and rep["clipped"] == 1
    want = a + (w - a) * 0.5
    if sigma:
        want = want + torch.tensor(g) * sigma
    assert _bits(got) == _bits(want)
    # first4: element i draws index 4 * first4 + i
    got = a.clone()
    pv.torch_privatize_(got, a, 1.0, 1.0, SEED, 2, 1, first4=3)
    assert _bits(got) == _bits(a + pv.torch_gauss(76, SEED, 2, 1)[12:])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_update_sends_the_anchor(bad):
    w, a = _vectors(seed=3)
    w[17] = bad
    sigma = pv.f32(0.01)
    got, sh = w.clone(), torch.zeros(64, dtype=torch.bfloat16)
    rep = pv.torch_privatize_(got, a, 0.5, sigma, SEED, 0, 4, shadow=sh)
    assert rep["clipped"] == 2 and rep["scale"] == 0.0 and not math.isfinite(rep["update_l2"])
    assert bool(torch.isfinite(got).all())
    assert _bits(got) == _bits(a + pv.torch_gauss(64, SEED, 0, 4) * sigma)
    assert torch.equal(sh, got.to(torch.bfloat16))
    got = w.clone()
    assert pv.torch_privatize_(got, a, 0.5, 0.0)["clipped"] == 2 and _bits(got) == _bits(a)
    # an overflowing (finite) update is a diverged client too
    big = a.clone()
    big[0] = 3e38
    big[1] = -3e38
    got = big.clone()
    assert pv.torch_privatize_(got, a, 0.5, 0.0)["clipped"] == 2 and _bits(got) == _bits(a)


def test_specification_refusals():
    w, a = _vectors()
    for kw in (dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan")), dict(clip=float("inf")), dict(clip=1e-60),
               dict(sigma=-1.0), dict(sigma=float("inf")), dict(sigma=float("nan"))):
        args = dict(dict(clip=1.0, sigma=0.0), **kw)
        with pytest.raises(ValueError):
            pv.torch_privatize_(w.clone(), a, **args)
    with pytest.raises(ValueError):
        pv.torch_privatize_(w.clone(), a[:32], 1.0, 0.0)
    with pytest.raises(ValueError):
        pv.torch_privatize_(w.double(), a.double(), 1.0, 0.0)


class _Arena:
    """A three-tensor arena with two pads: [0, 70) + pad to 128, [128, 130) + pad to 192, [192, 256)."""
    offsets = {"a": (0, (7, 10)), "b": (128, (2,)), "c": (192, (64,))}
    numel = 256


def test_pads_stay_plus_zero():
    assert pv.arena_pads(_Arena) == [(70, 128), (130, 192)]
    live = torch.zeros(256, dtype=torch.bool)
    for off, shape in _Arena.offsets.values():
        live[off:off + math.prod(shape)] = True
    w, a = _vectors(256, seed=5)
    w, a = w * live, a * live
    p = pv.Privatizer(clip=0.005, noise_multiplier=2.0, seed=SEED)
    got, sh = w.clone(), torch.ones(256, dtype=torch.bfloat16)
    rep = p.privatize_(got, a, 1, 0, 4, shadow=sh, arena=_Arena)
    assert rep is p.last and rep["clipped"] == 1 and rep["sigma"] == pv.f32(0.005) == p.sigma(4)
    assert not got[~live].view(torch.int32).any() and not sh[~live].view(torch.int16).any()   # +0, not -0
    want = w.clone()
    pv.torch_privatize_(want, a, 0.005, p.sigma(4), SEED, 0, 1)
    assert bool(want[~live].any())                                   # (pad positions consume noise indices)
    assert _bits(got[live]) == _bits(want[live]) and torch.equal(sh, got.to(torch.bfloat16))
    # without an arena nothing is reset
    got = w.clone()
    p.privatize_(got, a, 1, 0, 4)
    assert _bits(got) == _bits(want)
    # the default model arena: the classifier's 2-float bias leaves 62 pad floats
    model = models.DDoSClassifier(config=models.DistilBertConfig(n_layers=1), device="cpu", impl="torch", seed=0)
    pads = pv.arena_pads(model.arena)
    assert sum(b - a_ for a_, b in pads) == model.arena.numel - model.arena.n_params
    assert any(b - a_ == 62 for a_, b in pads)


def test_privatizer_seed_and_sigma():
    a, b = pv.Privatizer(1.0, 1.0), pv.Privatizer(1.0, 1.0)
    assert a.seed != b.seed and 0 <= a.seed < 1 << 64             # 64 bits of os.urandom each
    assert pv.Privatizer(1.0, 1.0, seed=7).seed == 7
    p = pv.Privatizer(0.3, 1.5, delta=1e-6, seed=1)
    assert p.sigma(1) == pv.f32(0.45) and p.sigma(9) == pv.f32(0.15) and pv.Privatizer(0.3, 0.0, seed=1).sigma(3) == 0.0
    assert p.epsilon(3) == pv.epsilon(3, 1.5, 1e-6)
    with pytest.raises(ValueError):
        p.sigma(0)
    for kw, match in ((dict(clip=0.0), "privacy_clip"), (dict(clip=float("inf")), "privacy_clip"),
                      (dict(noise_multiplier=-1.0), "privacy_noise"), (dict(delta=0.0), "privacy_delta"),
                      (dict(delta=1.0), "privacy_delta"), (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed")):
        with pytest.raises(ValueError, match=match):
            pv.Privatizer(**dict(dict(clip=1.0, noise_multiplier=1.0), **kw))


# ------------------------------------------------------------------ the accountant
def test_epsilon():
    for R, z, delta in ((1, 1.0, 1e-5), (3, 0.3, 1e-5), (10, 0.1, 1e-6), (100, 4.0, 1e-3), (7, 1.1, 0.5)):
        a, b = R / (2.0 * z * z), math.log(1.0 / delta)
        star = 1.0 + math.sqrt(b / a)
        alphas = 1.0 + (star - 1.0) * np.exp(np.linspace(-3.0, 3.0, 600001))   # a fine grid around the minimum
        brute = float(np.min(a * alphas + b / (alphas - 1.0)))
        eps = pv.epsilon(R, z, delta)
        assert brute >= eps * (1 - 1e-12) and brute <= eps * (1 + 1e-9), (R, z, delta)
    assert pv.epsilon(5, 0.0, 1e-5) == math.inf and pv.epsilon(0, 0.0, 1e-5) == 0.0
    eps = [pv.epsilon(R, 1.0, 1e-5) for R in range(1, 20)]
    assert all(x < y for x, y in zip(eps, eps[1:]))                     # monotone in R
    eps = [pv.epsilon(3, z, 1e-5) for z in (4.0, 2.0, 1.0, 0.5, 0.1, 0.01)]
    assert all(x < y for x, y in zip(eps, eps[1:]))                     # ... and in 1 / z
    assert pv.epsilon(3, 1.0, 1e-6) > pv.epsilon(3, 1.0, 1e-5)
    for bad in ((-1, 1.0, 1e-5), (1, -1.0, 1e-5), (1, 1.0, 0.0), (1, 1.0, 1.0), (1, float("nan"), 1e-5)):
        with pytest.raises(ValueError):
            pv.epsilon(*bad)


# ------------------------------------------------------------------ plumbing
def _cfg(outdir, rounds, **kw):
    base = dict(out_dir=outdir, synthetic_rows=600, data_fraction=0.1, max_len=32, epochs=1, batch_size=8,
                eval_batch_size=16, plots=False, resume=False, rounds=rounds, verbose=False, heartbeat_s=0.0,
                save_checkpoints=False)
    base.update(kw)
    return config.FedConfig(**base)


def _client(cfg, frame):
    return runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1)).setup()


def test_config_env_and_cli_reach_the_runner(monkeypatch, tmp_path):
    d = config.FedConfig()
    assert (d.privacy_clip, d.privacy_noise, d.privacy_delta, d.privacy_seed) == (0.0, 0.0, 1e-5, None)
    parser = config.FedConfig.add_cli(argparse.ArgumentParser())
    cfg = config.FedConfig.from_args(parser.parse_args(
        ["--privacy-clip", "0.5", "--privacy-noise", "1.1", "--privacy-delta", "1e-6", "--privacy-seed", "12345"]))
    assert (cfg.privacy_clip, cfg.privacy_noise, cfg.privacy_delta, cfg.privacy_seed) == (0.5, 1.1, 1e-6, 12345)
    env = (("FEDDDOS_PRIVACY_CLIP", "0.25"), ("FEDDDOS_PRIVACY_NOISE", "0.3"), ("FEDDDOS_PRIVACY_DELTA", "1e-4"),
           ("FEDDDOS_PRIVACY_SEED", str(SEED)))
    for k, v in env:
        monkeypatch.setenv(k, v)
    cfg = config.FedConfig.from_args(parser.parse_args([]))
    assert (cfg.privacy_clip, cfg.privacy_noise, cfg.privacy_delta, cfg.privacy_seed) == (0.25, 0.3, 1e-4, SEED)
    cfg = config.FedConfig.from_args(parser.parse_args(["--privacy-clip", "2"]))  # flags win
    assert cfg.privacy_clip == 2.0 and cfg.privacy_noise == 0.3
    _clear_rank_env()
    for k, v in dict(out_dir=str(tmp_path), synthetic_rows=600, max_len=32, plots=False, resume=False, verbose=False,
                     heartbeat_s=0.0).items():
        setattr(cfg, k, v)
    client = _client(cfg, None)
    p = client.privacy
    assert (p.clip, p.noise_multiplier, p.delta, p.seed) == (2.0, 0.3, 1e-4, SEED)
    for k, _ in env:
        monkeypatch.delenv(k)
    assert _client(_cfg(str(tmp_path), 1), None).privacy is None
    assert pv.make_privatizer(_cfg(str(tmp_path), 1)) is None and not pv.check_privacy_config(_cfg(str(tmp_path), 1))
    assert pv.make_privatizer(types.SimpleNamespace()) is None      # (a configuration from before the fields)
    # refused at setup, before any work, with a message naming the flag
    for kw, match in ((dict(privacy_clip=-1.0), "privacy_clip"), (dict(privacy_clip=float("inf")), "privacy_clip"),
                      (dict(privacy_clip=float("nan")), "privacy_clip"),
                      (dict(privacy_clip=1.0, privacy_noise=-0.1), "privacy_noise"),
                      (dict(privacy_clip=1.0, privacy_noise=float("inf")), "privacy_noise"),
                      (dict(privacy_noise=1.0), "privacy_noise.*privacy_clip"),
                      (dict(privacy_clip=1.0, privacy_delta=0.0), "privacy_delta"),
                      (dict(privacy_clip=1.0, privacy_delta=1.0), "privacy_delta"),
                      (dict(privacy_delta=-0.5), "privacy_delta"),
                      (dict(privacy_clip=1.0, privacy_seed=-1), "privacy_seed"),
                      (dict(privacy_clip=1.0, weighted_fedavg=True), "weighted_fedavg")):
        with pytest.raises(ValueError, match=match):
            _client(_cfg(str(tmp_path), 1, **kw), None)
    with pytest.raises(ValueError, match="gpus_per_client"):
        pv.make_privatizer(_cfg(str(tmp_path), 1, privacy_clip=1.0), gpus_per_client=2)
    with pytest.raises(ValueError, match="gpus_per_client"):
        pv.check_privacy_config(_cfg(str(tmp_path), 1, privacy_clip=1.0), 2)
    # a fresh seed per job unless one is fixed
    a = pv.make_privatizer(_cfg(str(tmp_path), 1, privacy_clip=1.0))
    b = pv.make_privatizer(_cfg(str(tmp_path), 1, privacy_clip=1.0))
    assert a.seed != b.seed and a.noise_multiplier == 0.0


def test_default_path_never_privatizes(tmp_path, monkeypatch):
    """2 virtual clients x 2 rounds and one real client's round, privacy_clip = 0: no call of
    ``privatize_``, no privacy key in any record."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)

    def boom(*a, **k):
        raise AssertionError("the default path reached the privatizer")

    monkeypatch.setattr(pv.Privatizer, "privatize_", boom)
    monkeypatch.setattr(pv, "torch_privatize_", boom)
    cfg = _cfg(str(tmp_path), 2)
    client = _client(cfg, frame)
    assert client.privacy is None
    res = _single_thread(lambda: runner.run_virtual_clients(client, 2, rounds=2))
    for h in res["rounds"]:
        assert not any(k.startswith("privacy") for k in h)
        for c in h["clients"]:
            assert not any(k in c for k in PRIVACY_KEYS) and not any(k.startswith("privacy") for k in c)
    # one real client, one round (run_round in a single process): the same
    solo = _client(_cfg(str(tmp_path / "solo"), 1), frame)
    rec = _single_thread(lambda: solo.run_round(0))
    assert not any(k in rec for k in PRIVACY_KEYS)
    assert "privacy_epsilon" not in solo.report()


# ------------------------------------------------------------------ end-to-end runs
def _fed_worker(rank, world, port, outdir, rounds, kw):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    comm.init_distributed(device="cpu")
    torch.set_num_threads(1)
    cfg = _cfg(outdir, rounds, **kw)
    frame = data_pkg.generate_cicids2017(cfg.synthetic_rows, seed=0)
    client = runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1))
    client.setup()
    for r in range(client.start_round, cfg.rounds):
        client.run_round(r)
    rep = client.report()
    torch.save({"master": client.model.arena.master.clone(), "history": client.history, "report": rep},
               os.path.join(outdir, f"state_rank{rank}.pt"))
    client.log.close()
    comm.shutdown()


def test_virtual_equals_two_rank_gloo_run(tmp_path):
    """tests/test_virtual_rounds.py's configuration with clip + noise under a fixed seed: the virtual
    run and the 2-rank gloo run agree bit for bit, records included."""
    world, rounds = 2, 2
    real = tmp_path / "real"
    real.mkdir()
    kw = dict(synthetic_rows=1500, max_len=64, privacy_clip=0.02, privacy_noise=0.5, privacy_seed=SEED)
    mp.spawn(_fed_worker, args=(world, _free_port(), str(real), rounds, kw), nprocs=world, join=True)
    _clear_rank_env()
    cfg = _cfg(str(tmp_path / "virtual"), rounds, **kw)
    frame = data_pkg.generate_cicids2017(cfg.synthetic_rows, seed=0)

    def virtual():
        client = _client(cfg, frame)
        init = client.model.arena.master.clone()
        return client, init, runner.run_virtual_clients(client, world, rounds=rounds)

    client, init, res = _single_thread(virtual)
    st = [torch.load(real / f"state_rank{r}.pt", weights_only=False) for r in range(world)]
    assert torch.equal(st[0]["master"], st[1]["master"])
    assert torch.equal(st[0]["master"], client.model.arena.master) and not torch.equal(init, st[0]["master"])
    sigma = pv.f32(0.5 * 0.02 / math.sqrt(2.0))
    for r in range(rounds):
        got = res["rounds"][r]
        assert got["privacy_epsilon"] == pv.epsilon(r + 1, 0.5, 1e-5)
        for rank in range(world):
            want, c = st[rank]["history"][r], got["clients"][rank]
            for k in PRIVACY_KEYS:
                assert c[k] == want[k], (rank, r, k)
            assert c["privacy_sigma"] == sigma and c["clipped"] in (0, 1) and c["update_l2"] > 0
            assert c["aggregated_test"]["loss"] == want["aggregated_test"]["loss"], (rank, r)
            assert c["local_test"]["loss"] == want["local_test"]["loss"], (rank, r)
    assert st[0]["report"]["privacy_epsilon"] == pv.epsilon(rounds, 0.5, 1e-5)
    assert st[0]["report"]["privacy_delta"] == 1e-5


def test_clip_only_bounds_the_aggregate(tmp_path):
    """A tiny C without noise: every client is clipped, and the aggregate -- a mean of updates of norm
    <= C -- stays within C (1 + 1e-5) of the round's start; the pads stay +0.  What a client sends,
    fl(a + fl(scale * d)), is within C of the start up to the roundings: 2^-24 relative for scale and
    for the product, and half an ulp of each sent weight for the sum (<= 2^-24 |sent| in norm)."""
    _clear_rank_env()
    C = 1e-2
    frame = data_pkg.generate_cicids2017(600, seed=0)
    client = _client(_cfg(str(tmp_path), 2, privacy_clip=C), frame)
    A = client.model.arena
    start = A.master.clone()
    live = torch.zeros(A.numel, dtype=torch.bool)
    for off, shape in A.offsets.values():
        live[off:off + math.prod(shape)] = True
    seen = []
    real = client.privacy.privatize_

    def spy(master, anchor, *a, **k):
        rep = real(master, anchor, *a, **k)
        seen.append((float((master.double() - anchor.double()).norm()), float(master.double().norm()),
                     bool(master[~live].view(torch.int32).any())))
        return rep

    client.privacy.privatize_ = spy
    for r in range(2):
        res = _single_thread(lambda: runner.run_virtual_clients(client, 3, rounds=1))
        h = res["rounds"][0]
        assert h["privacy_epsilon"] == math.inf                     # clipping alone is no privacy
        for c in h["clients"]:
            assert c["clipped"] == 1 and c["privacy_sigma"] == 0.0 and c["update_l2"] > C
        assert float((A.master - start).double().norm()) <= C * (1 + 1e-5)
        start = A.master.clone()
    assert len(seen) == 6 and all(n <= C * (1 + 1e-6) + 2.0 ** -24 * m and not pad for n, m, pad in seen)


@pytest.mark.parametrize("kw,keys", [(dict(aggregator="median"), ("trimmed_share", "k")),
                                     (dict(server_opt="adam", server_lr=0.01), ("delta_l2", "step_l2"))])
def test_composes_with_the_other_features(tmp_path, kw, keys):
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    client = _client(_cfg(str(tmp_path), 1, privacy_clip=0.01, privacy_noise=0.2, privacy_seed=SEED, **kw), frame)
    res = _single_thread(lambda: runner.run_virtual_clients(client, 3, rounds=1))
    h = res["rounds"][0]
    assert all(k in h for k in keys) and h["privacy_epsilon"] == pv.epsilon(1, 0.2, 1e-5)
    assert all(all(k in c for k in PRIVACY_KEYS) for c in h["clients"])
    assert bool(torch.isfinite(client.model.arena.master).all())


def test_privatize_then_poison_and_a_dropped_client_warns(tmp_path):
    """run_round in one process: the record carries the privacy keys, a liar lies after the
    privatizer ran, and a dropped sampled client is named in a warning."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    client = _client(_cfg(str(tmp_path), 1, privacy_clip=1e-3, privacy_noise=1.0, privacy_seed=SEED, poison_client=0,
                          poison_kind="scale", poison_scale=1.0, drop_client=0), frame)
    order, lines = [], []
    real_priv, real_poison = client.privacy.privatize_, runner.faults.poison_
    client.privacy.privatize_ = lambda *a, **k: (order.append("privatize"), real_priv(*a, **k))[1]
    client.log.info = lambda msg, *a, **k: lines.append(msg)
    try:
        runner.faults.poison_ = lambda *a, **k: (order.append("poison"), real_poison(*a, **k))[1]
        rec = _single_thread(lambda: client.run_round(0))
    finally:
        runner.faults.poison_ = real_poison
    assert order == ["privatize", "poison"]
    assert rec["clipped"] == 1 and rec["privacy_sigma"] == pv.f32(1e-3) and rec["update_l2"] > 1e-3
    assert rec["privacy_epsilon"] == pv.epsilon(1, 1.0, 1e-5)
    assert any("[WARN]" in m and "less noise" in m for m in lines)
    assert any("upper bound" in m for m in lines)
