"""Byzantine-robust aggregation on the CPU (parallel/robust.py: coordinate-wise trimmed mean / median,
Yin et al. ICML 2018): the torch specification against a hand-written per-coordinate loop, the median
identities, NaN / inf / signed-zero inputs, permutation invariance, the configuration plumbing and its
refusals, the untouched default path, the virtual run against the 3-rank gloo run bit for bit, a client
that lies (``utils/faults.py poison_``), a dropped client, and the composition with a server optimizer."""
import argparse
import dataclasses
import json
import math
import os
import socket
import struct
import types

import pytest
import torch
import torch.multiprocessing as mp

PKG = "detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd"

from importlib import import_module  # noqa: E402

config = import_module(f"{PKG}.config")
data_pkg = import_module(f"{PKG}.data")
models = import_module(f"{PKG}.models")
runner = import_module(f"{PKG}.fed.runner")
rb = import_module(f"{PKG}.parallel.robust")
so = import_module(f"{PKG}.parallel.server_opt")
faults = import_module(f"{PKG}.utils.faults")

NEW_FIELDS = ("aggregator", "trim_ratio", "poison_client", "poison_round", "poison_kind", "poison_scale")


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


class FlatModel:
    """What ``robust_aggregate_`` / ``ServerOptimizer`` need of a model: a flat fp32 master."""

    def __init__(self, master):
        self.arena = types.SimpleNamespace(master=master, shadow=None)
        self.synced = 0

    def sync_shadow(self, force=False):
        self.synced += 1

    def mark_shadow_synced(self):
        self.synced += 1


def _states(M, n=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = 0.05 * torch.randn(n, generator=g)
    return [base + 1e-3 * torch.randn(n, generator=g) for _ in range(M)]


# ------------------------------------------------------------------ the specification
def _key(x: float) -> int:
    b = struct.unpack("<i", struct.pack("<f", x))[0]
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _hand(states, k):
    """The specification per coordinate in plain Python: sort (key, slot), drop k at each end, add the
    rest ascending with every sum rounded to fp32, multiply by fp32(1 / (M - 2k))."""
    M, n = len(states), states[0].numel()
    inv = _f32(1.0 / (M - 2 * k))
    out, trimmed = [], [0] * M
    for i in range(n):
        vals = [struct.unpack("<f", struct.pack("<i", int(s.view(torch.int32)[i])))[0] for s in states]
        order = sorted(range(M), key=lambda j: (_key(vals[j]), j))
        for j in order[:k] + order[M - k:]:
            trimmed[j] += 1
        acc = vals[order[k]]
        for j in order[k + 1:M - k]:
            acc = _f32(acc + vals[j])
        out.append(_f32(acc * inv))
    return torch.tensor(out, dtype=torch.float32), trimmed


def _biteq(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("M", [2, 3, 4, 5, 8])
def test_torch_chain_equals_a_hand_written_loop(M):
    states = _states(M, seed=M)
    states[0][5] = states[1][5]          # a tie: broken by the slot index
    states[M - 1][9] = -states[0][9]
    for k in range((M - 1) // 2 + 1):
        out, trimmed, nonfinite = rb.torch_robust_(states, k)
        want, want_trimmed = _hand(states, k)
        assert _biteq(out, want), (M, k)
        assert trimmed.dtype == torch.int64 and trimmed.tolist() == want_trimmed, (M, k)
        assert sum(want_trimmed) == 2 * k * 64 and nonfinite == 0
    with pytest.raises(ValueError, match="2k"):
        rb.torch_robust_(states, (M - 1) // 2 + 1)
    with pytest.raises(ValueError, match="2k"):
        rb.torch_robust_(states, -1)


def test_median_identities():
    for M in (3, 5, 7):
        states = _states(M, seed=10 + M)
        out, _, _ = rb.torch_robust_(states, (M - 1) // 2)
        assert _biteq(out, torch.stack(states).median(dim=0).values), M
    for M in (2, 4, 8):
        states = _states(M, seed=20 + M)
        out, _, _ = rb.torch_robust_(states, (M - 1) // 2)
        srt = torch.stack(states).sort(dim=0).values
        assert _biteq(out, (srt[M // 2 - 1] + srt[M // 2]) * 0.5), M
    # k = 0: the mean, summed in sorted order
    states = _states(5, seed=3)
    out, trimmed, _ = rb.torch_robust_(states, 0)
    srt = torch.stack(states).sort(dim=0).values
    acc = srt[0].clone()
    for j in range(1, 5):
        acc = acc + srt[j]
    assert _biteq(out, acc * _f32(1 / 5)) and trimmed.tolist() == [0] * 5
    # one client is its own aggregate
    out, trimmed, _ = rb.torch_robust_(states[:1], 0)
    assert _biteq(out, states[0]) and trimmed.tolist() == [0]


def test_nan_inf_and_signed_zero():
    n = 64
    states = _states(5, n, seed=1)
    nan = float("nan")
    states[1] = torch.full((n,), nan)
    states[3] = -torch.full((n,), nan)  # the sign bit set: sorts below -inf
    assert bool(torch.signbit(states[3]).all())
    out, trimmed, nonfinite = rb.torch_robust_(states, 1)
    assert nonfinite == 0 and bool(torch.isfinite(out).all())
    assert trimmed.tolist() == [0, n, 0, n, 0]
    honest = [states[0], states[2], states[4]]
    assert _biteq(out, rb.torch_robust_(honest, 0)[0])
    # one bad client more than k covers: the NaN reaches the output and is counted
    out, trimmed, nonfinite = rb.torch_robust_(states, 0)
    assert nonfinite == n
    states[3] = torch.full((n,), float("-inf"))
    states[4] = torch.full((n,), float("inf"))
    out, trimmed, nonfinite = rb.torch_robust_(states, 2)  # NaN, -inf, +inf of 5: the median survives
    assert nonfinite == 0 and trimmed[1] == n and trimmed[3] == n and trimmed[4] == n
    out1, _, nonfinite1 = rb.torch_robust_(states, 1)
    assert nonfinite1 == n  # (-inf + finite + ... or +inf left in the sum)
    # -0 sorts below +0; an all +0 pad stays +0 with no bit set
    z = [torch.zeros(n), -torch.zeros(n), torch.zeros(n)]
    out, trimmed, _ = rb.torch_robust_(z, 1)
    assert not out.view(torch.int32).any() and trimmed.tolist() == [0, n, n]
    out, _, _ = rb.torch_robust_([torch.zeros(n)] * 4, 1)
    assert not out.view(torch.int32).any()
    out, _, _ = rb.torch_robust_([-torch.zeros(n)] * 3, 1)
    assert bool(torch.signbit(out).all())  # (the middle value times 1: -0 stays -0)


def test_permutation_invariance():
    states = _states(5, seed=4)
    states[2] = states[2] * -4.0
    perm = [3, 0, 4, 2, 1]
    for k in (0, 1, 2):
        a, ta, _ = rb.torch_robust_(states, k)
        b, tb, _ = rb.torch_robust_([states[p] for p in perm], k)
        assert _biteq(a, b), k
        assert [int(tb[perm.index(j)]) for j in range(5)] == ta.tolist(), k


# ------------------------------------------------------------------ configuration
def test_trim_count_and_refusals():
    assert [rb.trim_count(M, "median") for M in (1, 2, 3, 4, 5, 8, 16)] == [0, 0, 1, 1, 2, 3, 7]
    assert [rb.trim_count(M, "trimmed_mean", 0.2) for M in (1, 3, 5, 8, 10, 16)] == [0, 0, 1, 1, 2, 3]
    assert rb.trim_count(8, "trimmed_mean", 0.0) == 0 and rb.trim_count(8, "mean") == 0
    assert rb.trim_count(7, "trimmed_mean", 0.49) == 3
    for bad in (0.5, 0.75, -0.1, float("nan"), "x"):
        with pytest.raises(ValueError, match="trim_ratio"):
            rb.trim_count(8, "trimmed_mean", bad)
    with pytest.raises(ValueError, match="aggregator"):
        rb.trim_count(8, "krum")
    cfg = config.FedConfig()
    assert cfg.aggregator == "mean" and cfg.trim_ratio == 0.2 and rb.check_robust_config(cfg) is None
    assert rb.make_robust(cfg) is None
    assert (cfg.poison_client, cfg.poison_round, cfg.poison_kind, cfg.poison_scale) == (None, None, "scale", -4.0)
    assert rb.check_robust_config(config.FedConfig(aggregator="median")) == "median"
    assert rb.check_robust_config(config.FedConfig(aggregator="trimmed_mean", trim_ratio=0.1)) == "trimmed_mean"
    for kw, match in ((dict(aggregator="krum"), "aggregator"),
                      (dict(aggregator="median", transport="tcp"), "transport"),
                      (dict(aggregator="trimmed_mean", transport="tcp"), "transport"),
                      (dict(aggregator="median", weighted_fedavg=True), "weighted_fedavg"),
                      (dict(aggregator="trimmed_mean", trim_ratio=0.5), "trim_ratio"),
                      (dict(aggregator="trimmed_mean", trim_ratio=-0.01), "trim_ratio")):
        with pytest.raises(ValueError, match=match):
            rb.check_robust_config(config.FedConfig(**kw))
    # the plain mean keeps tcp and weighting
    assert rb.check_robust_config(config.FedConfig(transport="tcp", weighted_fedavg=True)) is None


def test_two_k_not_below_m_names_trim_ratio(monkeypatch):
    """``floor(trim_ratio * M) * 2 >= M`` cannot happen for a ratio in [0, 0.5); the guard behind the
    range check still names trim_ratio when the range check is out of the way."""
    monkeypatch.setattr(rb, "_check_ratio", float)
    with pytest.raises(ValueError, match="trim_ratio"):
        rb.trim_count(4, "trimmed_mean", 0.5)


def _cfg(outdir, rounds, **kw):
    base = dict(out_dir=outdir, synthetic_rows=600, data_fraction=0.1, max_len=32, epochs=1, batch_size=8,
                eval_batch_size=16, plots=False, resume=False, rounds=rounds, verbose=False, heartbeat_s=0.0,
                save_checkpoints=False)
    base.update(kw)
    return config.FedConfig(**base)


def _client(cfg, frame):
    return runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1)).setup()


def test_config_env_and_cli_reach_the_runner(monkeypatch, tmp_path):
    parser = config.FedConfig.add_cli(argparse.ArgumentParser())
    cfg = config.FedConfig.from_args(parser.parse_args(
        ["--aggregator", "trimmed_mean", "--trim-ratio", "0.25", "--poison-client", "1", "--poison-round", "0",
         "--poison-kind", "noise", "--poison-scale", "0.5"]))
    assert (cfg.aggregator, cfg.trim_ratio) == ("trimmed_mean", 0.25)
    assert (cfg.poison_client, cfg.poison_round, cfg.poison_kind, cfg.poison_scale) == (1, 0, "noise", 0.5)
    for k, v in (("FEDDDOS_AGGREGATOR", "median"), ("FEDDDOS_TRIM_RATIO", "0.1"), ("FEDDDOS_POISON_CLIENT", "2"),
                 ("FEDDDOS_POISON_ROUND", "1"), ("FEDDDOS_POISON_KIND", "nan"), ("FEDDDOS_POISON_SCALE", "-2")):
        monkeypatch.setenv(k, v)
    cfg = config.FedConfig.from_args(parser.parse_args([]))
    assert (cfg.aggregator, cfg.trim_ratio) == ("median", 0.1)
    assert (cfg.poison_client, cfg.poison_round, cfg.poison_kind, cfg.poison_scale) == (2, 1, "nan", -2.0)
    cfg = config.FedConfig.from_args(parser.parse_args(["--aggregator", "trimmed_mean"]))  # flags win
    assert cfg.aggregator == "trimmed_mean" and cfg.trim_ratio == 0.1
    _clear_rank_env()
    for k, v in dict(out_dir=str(tmp_path), synthetic_rows=600, max_len=32, plots=False, resume=False, verbose=False,
                     heartbeat_s=0.0).items():
        setattr(cfg, k, v)
    client = _client(cfg, None)
    assert client.robust.aggregator == "trimmed_mean" and client.robust.trim_ratio == 0.1
    assert client.robust.gpus_per_client == 1 and client.robust.k(8) == 0 and client.robust.k(10) == 1
    for k in ("FEDDDOS_AGGREGATOR", "FEDDDOS_TRIM_RATIO", "FEDDDOS_POISON_CLIENT", "FEDDDOS_POISON_ROUND",
              "FEDDDOS_POISON_KIND", "FEDDDOS_POISON_SCALE"):
        monkeypatch.delenv(k)
    assert _client(_cfg(str(tmp_path), 1), None).robust is None
    # refused at setup, before any work
    for kw, match in ((dict(aggregator="krum"), "aggregator"), (dict(aggregator="median", transport="tcp"), "transport"),
                      (dict(aggregator="median", weighted_fedavg=True), "weighted_fedavg")):
        with pytest.raises(ValueError, match=match):
            _client(_cfg(str(tmp_path), 1, **kw), None)


def test_poison_kinds():
    cfg = config.FedConfig(poison_client=1, poison_round=2)
    m = torch.arange(8, dtype=torch.float32)
    assert not faults.poison_(m, cfg, 0, 2) and not faults.poison_(m, cfg, 1, 1)
    assert torch.equal(m, torch.arange(8, dtype=torch.float32))
    assert faults.poison_(m, cfg, 1, 2) and torch.equal(m, -4.0 * torch.arange(8, dtype=torch.float32))
    cfg = config.FedConfig(poison_client=0, poison_kind="noise", poison_scale=-0.5)
    a, b, c = torch.zeros(4096), torch.zeros(4096), torch.zeros(4096)
    assert faults.poison_(a, cfg, 0, 0) and faults.poison_(b, cfg, 0, 0) and faults.poison_(c, cfg, 0, 1)
    assert torch.equal(a, b) and not torch.equal(a, c)  # seeded from (base_seed, client, round)
    assert abs(float(a.std()) - 0.5) < 0.05
    cfg = config.FedConfig(poison_client=0, poison_kind="nan")
    assert faults.poison_(a, cfg, 0, 7) and bool(torch.isnan(a).all())
    with pytest.raises(ValueError, match="poison_kind"):
        faults.poison_(a, config.FedConfig(poison_client=0, poison_kind="flip"), 0, 0)


# ------------------------------------------------------------------ the default path
class _NoNewFields:
    """A configuration as the parent commit knew it: the new fields do not exist."""

    def __init__(self, cfg):
        self.__dict__.update({f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg) if f.name not in NEW_FIELDS})

    def client_seed(self, client_id):
        return self.base_seed + client_id


def test_default_mean_is_bit_identical(tmp_path, monkeypatch):
    """tests/test_virtual_rounds.py's configuration, 2 clients x 2 rounds: ``aggregator="mean"`` against a
    configuration without the new fields -- and neither run reaches the robust code."""
    _clear_rank_env()
    kw = dict(synthetic_rows=1500, max_len=64)
    frame = data_pkg.generate_cicids2017(1500, seed=0)

    def boom(*a, **k):
        raise AssertionError("the default path reached the robust aggregate")

    monkeypatch.setattr(runner, "robust_aggregate_", boom)

    def run(cfg):
        client = _client(cfg, frame)
        res = runner.run_virtual_clients(client, 2, rounds=2)
        return client.model.arena.master.clone(), res

    cfg = _cfg(str(tmp_path), 2, **kw)
    assert all(hasattr(cfg, f) for f in NEW_FIELDS)
    old = _NoNewFields(cfg)
    assert not any(hasattr(old, f) for f in NEW_FIELDS)
    a, ra = _single_thread(lambda: run(cfg))
    b, rb_ = _single_thread(lambda: run(old))
    assert torch.equal(a, b)
    for x, y in zip(ra["rounds"], rb_["rounds"]):
        assert "trimmed_share" not in x and "k" not in x
        assert x["aggregated_confusion"] == y["aggregated_confusion"]
        assert [c["aggregated_test"]["loss"] for c in x["clients"]] == [c["aggregated_test"]["loss"] for c in y["clients"]]


# ------------------------------------------------------------------ collective runs
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
    torch.save({"master": client.model.arena.master.clone(), "history": client.history},
               os.path.join(outdir, f"state_rank{rank}.pt"))
    client.log.close()
    comm.shutdown()


def test_virtual_median_equals_three_rank_gloo_run(tmp_path):
    world, rounds = 3, 2
    real = tmp_path / "real"
    real.mkdir()
    kw = dict(aggregator="median")
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
    for s in st:
        assert torch.equal(s["master"], st[0]["master"])
    assert torch.equal(st[0]["master"], client.model.arena.master) and not torch.equal(init, st[0]["master"])
    for r in range(rounds):
        got = res["rounds"][r]
        assert got["k"] == 1 and len(got["trimmed_share"]) == 3
        assert abs(sum(got["trimmed_share"]) - 2.0) < 1e-9  # 2k values trimmed per coordinate
        for rank in range(world):
            want = st[rank]["history"][r]
            assert want["k"] == 1 and want["trimmed_share"] == got["trimmed_share"], (rank, r)
            assert got["clients"][rank]["aggregated_test"]["loss"] == want["aggregated_test"]["loss"], (rank, r)


def _flat_worker(rank, world, port, outdir, drop_rank, aggregator, with_server):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    fedavg = import_module(f"{PKG}.parallel.fedavg")
    comm.init_distributed(device="cpu")
    mine = _states(world, n=256, seed=11)[rank]
    model = FlatModel(mine.clone())
    server = so.ServerOptimizer(FlatModel(torch.zeros(256)), "adam", lr=0.01) if with_server else None
    robust = rb.RobustAggregator(aggregator, 0.2)
    total = fedavg.fedavg_(model, participate=rank != drop_rank, server=server, robust=robust)
    torch.save({"master": model.arena.master.clone(), "total": total, "last": robust.last,
                "synced": model.synced}, os.path.join(outdir, f"flat{rank}.pt"))
    comm.shutdown()


def test_dropped_client_with_median_at_four(tmp_path):
    """N = 4, client 3's update dropped: 3 rows enter (k = 1), and the dropped client receives the same
    aggregate as the others."""
    mp.spawn(_flat_worker, args=(4, _free_port(), str(tmp_path), 2, "median", False), nprocs=4, join=True)
    states = _states(4, n=256, seed=11)
    want, trimmed, _ = rb.torch_robust_([states[0], states[1], states[3]], 1)
    for rank in range(4):
        got = torch.load(tmp_path / f"flat{rank}.pt", weights_only=False)
        assert got["total"] == 3.0 and got["last"]["clients"] == 3 and got["last"]["k"] == 1, rank
        assert torch.equal(got["master"], want) and got["last"]["trimmed"] == trimmed.tolist(), rank
        assert got["synced"] == 1
    four, _, _ = rb.torch_robust_(states, 1)
    assert not torch.equal(four, want)


def test_nobody_participates_raises():
    model = FlatModel(torch.zeros(8))
    fedavg = import_module(f"{PKG}.parallel.fedavg")
    _clear_rank_env()
    # (one process: a client that does not participate returns 0, as the plain path does)
    assert fedavg.fedavg_(model, participate=False, robust=rb.RobustAggregator("median")) == 0.0
    assert fedavg.fedavg_(model, participate=True, robust=rb.RobustAggregator("median")) == 1.0


# ------------------------------------------------------------------ a client that lies
def test_nan_poisoner_breaks_the_mean_and_not_the_median(tmp_path, monkeypatch):
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    poison = dict(poison_client=1, poison_kind="nan")

    def run(**kw):
        client = _client(_cfg(str(tmp_path), 1, **poison, **kw), frame)
        res = runner.run_virtual_clients(client, 3, rounds=1)
        return client.model.arena.master.clone(), res

    # the hole: the plain mean adopts the poisoner's NaNs without a word
    mean, _ = _single_thread(lambda: run())
    assert not bool(torch.isfinite(mean).any())
    seen = []
    real = runner.robust_aggregate_

    def spy(model, states, k, server=None):
        seen.append(([s.clone() for s in states], k))
        return real(model, states, k, server)

    monkeypatch.setattr(runner, "robust_aggregate_", spy)
    med, res = _single_thread(lambda: run(aggregator="median"))
    assert bool(torch.isfinite(med).all())
    (states, k), = seen
    assert k == 1 and len(states) == 3 and bool(torch.isnan(states[1]).all())
    assert bool(torch.isfinite(states[0]).all()) and bool(torch.isfinite(states[2]).all())
    want, trimmed, nonfinite = rb.torch_robust_(states, 1)
    assert torch.equal(med, want) and nonfinite == 0
    rec = res["rounds"][0]
    assert rec["k"] == 1 and rec["trimmed_share"][1] == 1.0
    assert rec["trimmed_share"] == [int(t) / med.numel() for t in trimmed]
    # trimmed_mean 0.2 of 3 clients trims nobody: the NaNs come through and the round refuses them
    with pytest.raises(RuntimeError, match="non-finite"):
        _single_thread(lambda: run(aggregator="trimmed_mean"))


def test_one_poisoner_too_many_raises():
    states = _states(3, n=128, seed=5)
    states[0] = torch.full((128,), float("nan"))
    states[2] = torch.full((128,), float("nan"))
    model = FlatModel(torch.zeros(128))
    # (sorted: the honest value, NaN, NaN -- k = 1 drops the honest value and one NaN, the other stays)
    with pytest.raises(RuntimeError, match=r"non-finite.*slot 1 \(1\.000\), slot 2 \(1\.000\)"):
        rb.robust_aggregate_(model, states, 1)
    # with a server optimizer no step is made with the NaN aggregate
    srv = so.ServerOptimizer(FlatModel(torch.zeros(128)), "adam", lr=0.01)
    with pytest.raises(RuntimeError, match="non-finite"):
        rb.robust_aggregate_(model, states, 1, srv)
    assert srv.rounds == 0 and not srv.m.any() and bool(torch.isfinite(srv.x).all())
    with pytest.raises(ValueError, match="2k"):
        rb.robust_aggregate_(model, states, 2)
    with pytest.raises(ValueError, match="no participating"):
        rb.robust_aggregate_(model, [], 0)


# ------------------------------------------------------------------ server optimizer
def test_composes_with_server_adam():
    n = 2048
    g = torch.Generator().manual_seed(9)
    x0 = 0.05 * torch.randn(n, generator=g)
    states = [x0 + 1e-3 * torch.randn(n, generator=g) for _ in range(5)]
    states[3] = states[3] * -4.0
    model = FlatModel(x0.clone())
    srv = so.ServerOptimizer(model, "adam", lr=0.01, betas=(0.9, 0.99), tau=1e-3)
    rep = rb.robust_aggregate_(model, states, 2, srv)
    agg, trimmed, _ = rb.torch_robust_(states, 2)
    x, m = x0.clone(), torch.zeros(n)
    v = torch.full((n,), so.f32(so.f32(1e-3) * so.f32(1e-3)))
    d, dx = so.torch_chain_("adam", agg, x, m, v, 1.0, so.f32(0.01), so.f32(0.9), so.f32(0.99), so.f32(1e-3))
    assert torch.equal(model.arena.master, x) and torch.equal(srv.x, x)
    assert torch.equal(srv.m, m) and torch.equal(srv.v, v) and srv.rounds == 1
    assert rep["trimmed"] == trimmed.tolist() and rep["k"] == 2 and rep["clients"] == 5 and rep["nonfinite"] == 0
    assert rep["trimmed_share"] == [t / n for t in rep["trimmed"]]
    assert srv.last["delta_l2"] == math.sqrt(float(d.double().square().sum()))
    assert model.synced == 1  # (the server step refreshes the shadow, once)
    # without a server: the aggregate itself, shadow refreshed once
    model2 = FlatModel(x0.clone())
    rep2 = rb.robust_aggregate_(model2, states, 2)
    assert torch.equal(model2.arena.master, agg) and model2.synced == 1 and rep2 == rep
    assert rb.most_trimmed(rep)[0] == 3 and rb.most_trimmed(rep)[1] > 0.9
