"""FedOpt server optimizers on the CPU (parallel/server_opt.py: FedAvgM / FedAdagrad / FedAdam /
FedYogi, Reddi et al. ICLR 2021): the fp32 torch chain against a hand-written loop, closed forms of
the first round, the untouched default path, the virtual run against the 2-rank gloo run bit for bit,
a dropped client, kill-and-resume with the server moments, the configuration plumbing and the FedProx
anchor after a server step."""
import argparse
import json
import math
import os
import shutil
import socket
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
so = import_module(f"{PKG}.parallel.server_opt")
ck = import_module(f"{PKG}.utils.checkpoint")

KINDS = ("avgm", "adagrad", "adam", "yogi")


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
    """What ``ServerOptimizer`` needs of a model: a flat fp32 master (no shadow on the CPU)."""

    def __init__(self, master):
        self.arena = types.SimpleNamespace(master=master, shadow=None)
        self.synced = 0

    def sync_shadow(self, force=False):
        self.synced += 1

    def mark_shadow_synced(self):
        self.synced += 1


def small(seed=0):
    return models.DDoSClassifier(config=models.DistilBertConfig(n_layers=1), seed=seed)


# ------------------------------------------------------------------ arithmetic
def _t(x):
    return torch.tensor(x, dtype=torch.float32)


def _hand_step(kind, s, x, m, v, inv, eta, b1, b2, tau):
    """One server step written out per tensor in fp32 torch ops, every scalar an fp32 0-dim tensor:
    the specification's lines in their order.  Returns (x', m', v')."""
    inv, eta, b1, b2, tau = _t(inv), _t(eta), _t(b1), _t(b2), _t(tau)
    one = _t(1.0)
    avg = s * inv
    d = avg - x
    if kind == "avgm":
        m = m * b1 + d
        return x + m * eta, m, None
    m = m * b1 + d * (one - b1)
    d2 = d * d
    if kind == "adagrad":
        v = v + d2
    elif kind == "adam":
        v = v * b2 + d2 * (one - b2)
    else:
        v = v - (d2 * (one - b2)) * torch.sign(v - d2)
    return x + (m * eta) / (torch.sqrt(v) + tau), m, v


@pytest.mark.parametrize("kind", KINDS)
def test_three_rounds_equal_a_hand_written_loop(kind):
    """3 rounds on a 2 048-element vector, held as four 'parameter tensors' by the hand-written side:
    ``ServerOptimizer.apply_`` (CPU) gives the same bits -- it is the same op order."""
    n, N = 2048, 3
    g = torch.Generator().manual_seed(7)
    x0 = 0.05 * torch.randn(n, generator=g)
    x0[100:164] = 0.0  # an alignment pad
    eta = 1.0 if kind == "avgm" else 0.01
    model = FlatModel(x0.clone())
    srv = so.ServerOptimizer(model, kind, lr=eta, betas=(0.9, 0.99), tau=1e-3)
    assert torch.equal(srv.x, x0) and not srv.m.any() and srv.rounds == 0
    if kind == "avgm":
        assert srv.v is None
    else:
        assert torch.equal(srv.v, torch.full((n,), 1e-3, dtype=torch.float32) ** 2)
    cuts = [0, 512, 700, 1500, n]
    hx = [x0[a:b].clone() for a, b in zip(cuts, cuts[1:])]
    hm = [torch.zeros(b - a) for a, b in zip(cuts, cuts[1:])]
    hv = [torch.full((b - a,), 1e-3, dtype=torch.float32) ** 2 for a, b in zip(cuts, cuts[1:])]
    for rnd in range(3):
        noise = 1e-3 * torch.randn(n, generator=g)
        noise[100:164] = 0.0
        s = N * (srv.x + noise)
        model.arena.master.copy_(s)
        want_d = (s * _t(1.0 / 3.0) - srv.x).double()
        x_before = srv.x.clone()
        norms = srv.apply_(model, float(N))
        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            hx[i], hm[i], hv[i] = _hand_step(kind, s[a:b], hx[i], hm[i], hv[i], 1.0 / 3.0, eta, 0.9, 0.99, 1e-3)
        assert torch.equal(srv.x, torch.cat(hx)), (kind, rnd)
        assert torch.equal(srv.m, torch.cat(hm)), (kind, rnd)
        if kind != "avgm":
            assert torch.equal(srv.v, torch.cat(hv)), (kind, rnd)
        assert torch.equal(model.arena.master, srv.x) and srv.rounds == rnd + 1
        # the pad stays +0 (sign bit included), by arithmetic
        for t in (srv.x, srv.m, model.arena.master):
            pad = t[100:164]
            assert not pad.any() and not torch.signbit(pad).any()
        assert norms["delta_l2"] == math.sqrt(float(want_d.square().sum()))
        assert norms["step_l2"] == math.sqrt(float((srv.x - x_before).double().square().sum()))
        assert norms == srv.last
    assert model.synced == 3


def test_round_one_closed_forms():
    n = 2048
    g = torch.Generator().manual_seed(3)
    x0 = 0.05 * torch.randn(n, generator=g)
    # avgm, lr 1, b1 0: m = d, so x' = x + (avg - x)
    a, b = x0 + 0.01 * torch.randn(n, generator=g), x0 + 0.01 * torch.randn(n, generator=g)
    model = FlatModel((a + b).clone())
    srv = so.ServerOptimizer(FlatModel(x0.clone()), "avgm", lr=1.0, betas=(0.0, 0.99))
    srv.apply_(model, 2.0)
    avg = (a + b) * 0.5
    assert torch.equal(srv.x, x0 + (avg - x0)) and torch.equal(model.arena.master, srv.x)
    # adam, round 1: m = (1 - b1) d and v = b2 tau^2 + (1 - b2) d^2, so
    #   x' - x = eta (1 - b1) d / (sqrt(b2 tau^2 + (1 - b2) d^2) + tau)
    # and for |d| >> tau every element moves by eta (1 - b1) / sqrt(1 - b2), whatever |d| is
    eta, b1, b2, tau = 0.01, 0.9, 0.99, 1e-6
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    d = sign * (0.1 + torch.rand(n, generator=g))  # |d| in [0.1, 1.1): >= 1e5 tau
    s = x0 + d
    model = FlatModel(s.clone())
    srv = so.ServerOptimizer(FlatModel(x0.clone()), "adam", lr=eta, betas=(b1, b2), tau=tau)
    srv.apply_(model, 1.0)
    dd = s.double() - x0.double()  # the pseudo-gradient, fp64
    exact = eta * (1 - b1) * dd / (torch.sqrt(b2 * tau * tau + (1 - b2) * dd * dd) + tau)
    moved = srv.x.double() - x0.double()
    # fp32 evaluation of a handful of ops on O(0.01) steps added to O(0.1) weights: a few ulp of x
    assert (moved - exact).abs().max() <= 4 * 2.0 ** -24 * float(x0.abs().max() + 0.011)
    bound = eta * (1 - b1) / math.sqrt(1 - b2)  # = 0.01
    rel = (moved.abs() / bound - 1).abs().max()
    assert rel < 1e-3, rel  # tau / (sqrt(1 - b2) |d|) <= 1e-4, plus fp32 rounding of x' - x (~1e-5 / 0.01)


# ------------------------------------------------------------------ default path
def _fedavg_worker(rank, world, port, outdir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist
    comm = import_module(f"{PKG}.parallel.comm")
    fedavg = import_module(f"{PKG}.parallel.fedavg")
    comm.init_distributed(device="cpu")
    torch.set_num_threads(1)
    res = {}
    for weights, tag in (((1.0, 1.0), "plain"), ((3.0, 5.0), "weighted")):
        model = small(seed=rank)
        mine = model.arena.master.clone()
        both = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(both, mine)
        total = fedavg.fedavg_(model, weight=weights[rank])
        # the parent's arithmetic, spelled out: pre-scale, sum, one multiplication by 1 / total
        want = (both[0] * weights[0] if weights[0] != 1.0 else both[0].clone())
        want.add_(both[1] * weights[1] if weights[1] != 1.0 else both[1])
        want.mul_(1.0 / sum(weights))
        res[tag] = (bool(torch.equal(model.arena.master, want)) and total == sum(weights)
                    and not torch.equal(both[0], both[1]))
        # the same exchange with a server optimizer (x = the seed-0 weights on both ranks): the step
        # is taken from the same weighted sum
        model, ref = small(seed=0), small(seed=0)
        srv = so.ServerOptimizer(model, "yogi", lr=0.01)
        model.arena.master.copy_(mine)
        fedavg.fedavg_(model, weight=weights[rank], server=srv)
        srv2 = so.ServerOptimizer(ref, "yogi", lr=0.01)
        sum_ = (both[0] * weights[0] if weights[0] != 1.0 else both[0].clone())
        sum_.add_(both[1] * weights[1] if weights[1] != 1.0 else both[1])
        ref.arena.master.copy_(sum_)
        srv2.apply_(ref, sum(weights))
        res[tag + "_server"] = bool(torch.equal(model.arena.master, ref.arena.master)
                                    and torch.equal(srv.m, srv2.m) and torch.equal(srv.v, srv2.v)
                                    and torch.equal(srv.x, model.arena.master))
    with open(os.path.join(outdir, f"fedavg{rank}.json"), "w") as f:
        json.dump(res, f)
    comm.shutdown()


def test_default_path_is_the_parents_fedavg(tmp_path):
    cfg = config.FedConfig()
    assert cfg.server_opt == "fedavg" and cfg.server_lr == 1.0 and cfg.server_betas == (0.9, 0.99)
    assert cfg.server_tau == 1e-3
    assert so.make_server_optimizer(small(), cfg) is None
    mp.spawn(_fedavg_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        res = json.load(open(tmp_path / f"fedavg{rank}.json"))
        assert res == {"plain": True, "weighted": True, "plain_server": True, "weighted_server": True}, (rank, res)


# ------------------------------------------------------------------ runner: collective runs
def _cfg(outdir, rounds, **kw):
    base = dict(out_dir=outdir, synthetic_rows=1500, data_fraction=0.1, max_len=64, epochs=1, batch_size=8,
                eval_batch_size=16, plots=False, resume=False, rounds=rounds, verbose=False, heartbeat_s=0.0)
    base.update(kw)
    return config.FedConfig(**base)


def _fed_worker(rank, world, port, outdir, rounds, kw, fixed_order):
    """One rank of a collective run; leaves its final weights and server state in state_rank<r>.pt.
    fixed_order: no shuffling (with dropout off in ``kw``, a round's local training then depends on its
    starting weights alone -- what a restarted process can reproduce)."""
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    comm = import_module(f"{PKG}.parallel.comm")
    comm.init_distributed(device="cpu")
    torch.set_num_threads(1)
    cfg = _cfg(outdir, rounds, **kw)
    frame = data_pkg.generate_cicids2017(cfg.synthetic_rows, seed=0)
    client = runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1))
    client.setup()
    if fixed_order:
        client.train_loader.shuffle = False
    for r in range(client.start_round, cfg.rounds):
        client.run_round(r)
    srv = client.server
    torch.save({"master": client.model.arena.master.clone(), "x": srv.x.clone(), "m": srv.m.clone(),
                "v": None if srv.v is None else srv.v.clone(), "rounds": srv.rounds,
                "start_round": client.start_round}, os.path.join(outdir, f"state_rank{rank}.pt"))
    client.log.close()
    comm.shutdown()


def _states(outdir, world=2):
    return [torch.load(os.path.join(outdir, f"state_rank{r}.pt"), weights_only=True) for r in range(world)]


def _same_state(a, b):
    return (torch.equal(a["master"], b["master"]) and torch.equal(a["x"], b["x"]) and torch.equal(a["m"], b["m"])
            and torch.equal(a["v"], b["v"]) and a["rounds"] == b["rounds"])


ADAM = dict(server_opt="adam", server_lr=0.01)


def test_virtual_run_equals_gloo_run_bitwise(tmp_path):
    """server_opt="adam" on tests/test_virtual_rounds.py's configuration: 2 ranks x 2 rounds over gloo
    == ``run_virtual_clients(2, 2)`` bit for bit; round 2 starts from round 1's server step."""
    world, rounds = 2, 2
    real = tmp_path / "real"
    real.mkdir()
    mp.spawn(_fed_worker, args=(world, _free_port(), str(real), rounds, ADAM, False), nprocs=world, join=True)
    _clear_rank_env()
    cfg = _cfg(str(tmp_path / "virtual"), rounds, save_checkpoints=False, **ADAM)
    frame = data_pkg.generate_cicids2017(cfg.synthetic_rows, seed=0)

    def virtual():
        client = runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1)).setup()
        init = client.model.arena.master.clone()
        return client, init, runner.run_virtual_clients(client, world, rounds=rounds)

    client, init, res = _single_thread(virtual)
    srv = client.server
    assert srv is not None and srv.kind == "adam" and srv.rounds == rounds
    st = _states(str(real))
    assert _same_state(st[0], st[1])
    mine = {"master": client.model.arena.master, "x": srv.x, "m": srv.m, "v": srv.v, "rounds": srv.rounds}
    assert _same_state(st[0], mine)
    assert torch.equal(srv.x, client.model.arena.master) and not torch.equal(srv.x, init)
    g = torch.load(real / "ddos_distilbert_model.pth", weights_only=True)
    sd = client.model.state_dict()
    assert set(g) == set(sd)  # (the global checkpoint holds the model's keys and nothing of the server's)
    for key in g:
        assert torch.equal(g[key], sd[key].to(g[key].dtype)), key
    for cid in range(1, world + 1):
        hist = json.load(open(real / f"client{cid}_fed_state.json"))["history"]
        for r in range(rounds):
            want, got = hist[r], res["rounds"][r]
            assert got["delta_l2"] == want["delta_l2"] > 0 and got["step_l2"] == want["step_l2"] > 0, (cid, r)
            c = got["clients"][cid - 1]
            assert c["aggregated_test"]["loss"] == want["aggregated_test"]["loss"], (cid, r)
            assert c["train"]["epoch_losses"] == want["train"]["epoch_losses"], (cid, r)
    # FedAdam moves every weight by at most ~ eta (1 - b1) / sqrt(1 - b2) = eta in round 1
    assert res["rounds"][0]["step_l2"] <= 0.01 * math.sqrt(init.numel())
    # the server state on disk is the final one
    saved = torch.load(ck.server_opt_path(str(real)), weights_only=True)
    assert saved["kind"] == "adam" and saved["rounds"] == rounds
    assert torch.equal(saved["m"], srv.m) and torch.equal(saved["v"], srv.v) and "x" not in saved


def test_dropped_client_stays_in_sync(tmp_path):
    """Client 2's update is dropped in round 1 (weight 0): it still makes the server step, so both ranks
    end with identical weights and identical m / v."""
    kw = dict(ADAM, drop_client=1, drop_round=0, synthetic_rows=600, max_len=32)
    mp.spawn(_fed_worker, args=(2, _free_port(), str(tmp_path), 2, kw, False), nprocs=2, join=True)
    st = _states(str(tmp_path))
    assert _same_state(st[0], st[1]) and st[0]["rounds"] == 2
    assert torch.equal(st[0]["x"], st[0]["master"]) and st[0]["m"].any()
    hist = [json.load(open(tmp_path / f"client{c}_fed_state.json"))["history"] for c in (1, 2)]
    assert [h["participated"] for h in hist[1]] == [False, True]
    assert hist[0][0]["delta_l2"] == hist[1][0]["delta_l2"] > 0


NO_DROPOUT = dict(hidden_dropout=0.0, attention_dropout=0.0, head_dropout=0.0)


def test_kill_and_resume_restores_the_server_moments(tmp_path, monkeypatch):
    """Two rounds straight against: round 1, rank 0 killed after FedAvg (aggregate, server state and
    round tag on disk -- ``faults`` hook), restart, round 2.  Final weights and server m / v are
    bit-equal on every rank.  (Dropout off and a fixed batch order: a round's local training then
    depends on its starting weights alone, as a restarted process needs.)  Then: the state file gone,
    or of another kind, with the round tag present -> setup fails."""
    kw = dict(ADAM, synthetic_rows=600, max_len=32, resume=True, **NO_DROPOUT)
    straight, broken = tmp_path / "straight", tmp_path / "broken"
    straight.mkdir()
    broken.mkdir()
    mp.spawn(_fed_worker, args=(2, _free_port(), str(straight), 2, kw, True), nprocs=2, join=True)
    monkeypatch.setenv("FEDDDOS_KILL_CLIENT", "0")
    monkeypatch.setenv("FEDDDOS_KILL_ROUND", "0")
    monkeypatch.setenv("FEDDDOS_KILL_AT", "post_fedavg")
    with pytest.raises(Exception, match="exit code 17|terminated"):
        mp.spawn(_fed_worker, args=(2, _free_port(), str(broken), 2, kw, True), nprocs=2, join=True)
    assert (broken / ".killed_client0_round0_r0").exists()
    assert json.load(open(broken / "ddos_distilbert_model.json"))["round"] == 1
    assert os.path.exists(ck.server_opt_path(str(broken))) and not (broken / "state_rank0.pt").exists()
    mp.spawn(_fed_worker, args=(2, _free_port(), str(broken), 2, kw, True), nprocs=2, join=True)  # (one-shot kill)
    for k in ("FEDDDOS_KILL_CLIENT", "FEDDDOS_KILL_ROUND", "FEDDDOS_KILL_AT"):
        monkeypatch.delenv(k)
    a, b = _states(str(straight)), _states(str(broken))
    assert [s["start_round"] for s in a] == [0, 0] and [s["start_round"] for s in b] == [1, 1]
    assert _same_state(a[0], a[1]) and _same_state(b[0], b[1])
    assert _same_state(a[0], b[0]) and a[0]["rounds"] == 2 and a[0]["m"].any()

    # a third round cannot start without the moments of round 2's aggregate
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)

    def setup(outdir, **over):
        cfg = _cfg(str(outdir), 3, **dict(kw, **over))
        return runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1)).setup()

    ok = setup(broken)
    assert ok.start_round == 2 and ok.server.rounds == 2 and torch.equal(ok.server.m, b[0]["m"])
    assert torch.equal(ok.server.v, b[0]["v"]) and torch.equal(ok.server.x, b[0]["master"])
    with pytest.raises(RuntimeError, match="kind 'adam'.*'yogi'"):
        setup(broken, server_opt="yogi")
    assert setup(broken, server_opt="fedavg").server is None  # (plain FedAvg needs no server state)
    gone = tmp_path / "gone"
    shutil.copytree(broken, gone)
    os.remove(ck.server_opt_path(str(gone)))
    with pytest.raises(RuntimeError, match="ddos_distilbert_server_opt.pth is missing"):
        setup(gone)
    assert setup(gone, resume=False).server.rounds == 0  # an explicit fresh start is allowed


# ------------------------------------------------------------------ configuration
class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def test_config_plumbing(monkeypatch, tmp_path):
    parser = config.FedConfig.add_cli(argparse.ArgumentParser())
    cfg = config.FedConfig.from_args(parser.parse_args(
        ["--server-opt", "yogi", "--server-lr", "0.003", "--server-betas", "0.8", "0.95", "--server-tau", "0.01"]))
    assert (cfg.server_opt, cfg.server_lr, cfg.server_betas, cfg.server_tau) == ("yogi", 0.003, (0.8, 0.95), 0.01)
    m = small()
    log = _Log()
    srv = so.make_server_optimizer(m, cfg, log=log)
    assert srv.kind == "yogi" and srv.adaptive and not log.lines
    assert (srv.lr, srv.b1, srv.b2, srv.tau) == tuple(so.f32(v) for v in (0.003, 0.8, 0.95, 0.01))
    assert torch.equal(srv.x, m.arena.master) and srv.x.data_ptr() != m.arena.master.data_ptr()
    assert torch.equal(srv.v, torch.full_like(srv.v, so.f32(so.f32(0.01) * so.f32(0.01))))
    for k, v in (("FEDDDOS_SERVER_OPT", "avgm"), ("FEDDDOS_SERVER_LR", "0.5"), ("FEDDDOS_SERVER_BETAS", "0.7,0.9"),
                 ("FEDDDOS_SERVER_TAU", "0.002")):
        monkeypatch.setenv(k, v)
    cfg = config.FedConfig.from_args(parser.parse_args([]))
    assert (cfg.server_opt, cfg.server_lr, cfg.server_betas, cfg.server_tau) == ("avgm", 0.5, (0.7, 0.9), 0.002)
    srv = so.make_server_optimizer(m, cfg)
    assert srv.kind == "avgm" and srv.v is None and srv.lr == 0.5 and srv.b1 == so.f32(0.7)
    # the runner's client builds it from the configuration (and flags win over the environment)
    _clear_rank_env()
    cfg = config.FedConfig.from_args(parser.parse_args(["--server-opt", "adam", "--server-lr", "1.0"]))
    for k, v in dict(out_dir=str(tmp_path), synthetic_rows=600, max_len=32, plots=False, resume=False, verbose=False,
                     heartbeat_s=0.0).items():
        setattr(cfg, k, v)
    client = runner.FederatedClient(cfg, model_config=models.DistilBertConfig(n_layers=1)).setup()
    assert client.server.kind == "adam" and client.server.lr == 1.0 and client.server.tau == so.f32(0.002)
    assert torch.equal(client.server.x, client.model.arena.master)
    # an adaptive kind at server_lr >= 1 is warned about; avgm at 1.0 is the sensible default
    log = _Log()
    so.make_server_optimizer(m, config.FedConfig(server_opt="adagrad"), log=log)
    assert len(log.lines) == 1 and "server_lr" in log.lines[0]
    so.make_server_optimizer(m, config.FedConfig(server_opt="avgm"), log=log)
    so.make_server_optimizer(m, config.FedConfig(server_opt="adagrad", server_lr=0.1), log=log)
    assert len(log.lines) == 1
    # warm_start leaves the server state reset at the warm weights
    client.server.m.fill_(1.0)
    client.server.rounds = 5
    runner.warm_start(client, epochs=1, rows=600)
    assert not client.server.m.any() and client.server.rounds == 0
    assert torch.equal(client.server.x, client.model.arena.master)
    assert torch.equal(client.server.v, torch.full_like(client.server.v, so.f32(so.f32(0.002) ** 2)))


@pytest.mark.parametrize("kw, match", [
    (dict(server_opt="sgd"), "server_opt"),
    (dict(server_opt="adam", server_lr=0.0), "server_lr"),
    (dict(server_opt="adam", server_lr=float("nan")), "server_lr"),
    (dict(server_opt="adam", server_lr=float("inf")), "server_lr"),
    (dict(server_opt="yogi", server_tau=0.0), "server_tau"),
    (dict(server_opt="yogi", server_tau=-1e-3), "server_tau"),
    (dict(server_opt="avgm", server_betas=(1.0, 0.99)), "server_betas"),
    (dict(server_opt="adam", server_betas=(0.9, -0.1)), "server_betas"),
    (dict(server_opt="adam", server_betas=(0.9,)), "server_betas"),
    (dict(server_opt="adam", transport="tcp"), "transport"),
])
def test_bad_configurations_raise(kw, match, tmp_path):
    with pytest.raises(ValueError, match=match):
        so.make_server_optimizer(small(), config.FedConfig(**kw))
    _clear_rank_env()
    cfg = _cfg(str(tmp_path), 1, **kw)
    with pytest.raises(ValueError, match=match):  # refused at setup, before any work
        runner.FederatedClient(cfg, frame=None, model_config=models.DistilBertConfig(n_layers=1)).setup()


def test_state_dict_round_trip():
    m = small()
    srv = so.ServerOptimizer(m, "adam", lr=0.01)
    m.arena.master.mul_(2.0)
    srv.apply_(m, 2.0)
    sd = srv.state_dict()
    assert sorted(sd) == ["betas", "kind", "lr", "m", "rounds", "tau", "v"] and sd["rounds"] == 1
    other = so.ServerOptimizer(m, "adam", lr=0.01)
    assert not other.m.any()
    other.load_state_dict(sd)
    assert torch.equal(other.m, srv.m) and torch.equal(other.v, srv.v) and other.rounds == 1
    assert torch.equal(other.x, m.arena.master)
    with pytest.raises(ValueError, match="kind"):
        so.ServerOptimizer(m, "adagrad", lr=0.01).load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        so.ServerOptimizer(m, "avgm").load_state_dict(sd)
    sd["m"] = sd["m"][:-64]
    with pytest.raises(ValueError, match="fit"):
        other.load_state_dict(sd)


# ------------------------------------------------------------------ FedProx interplay
def test_fedprox_anchor_is_the_server_step(tmp_path, monkeypatch):
    """prox_mu > 0 with a server optimizer: ``ArenaAdam`` snapshots its anchor from the master at
    ``reset_state()``, after the server step -- round 2's anchors are the server's x, bit for bit."""
    _clear_rank_env()
    frame = data_pkg.generate_cicids2017(600, seed=0)
    opts, xs = [], []
    make, average = runner.make_optimizer, runner._average_masters

    def spy_make(model, cfg, *a, **kw):
        opts.append(make(model, cfg, *a, **kw))
        return opts[-1]

    def spy_average(model, states, server=None):
        out = average(model, states, server)
        xs.append(server.x.detach().clone())
        return out

    monkeypatch.setattr(runner, "make_optimizer", spy_make)
    monkeypatch.setattr(runner, "_average_masters", spy_average)
    cfg = _cfg(str(tmp_path), 2, synthetic_rows=600, max_len=32, save_checkpoints=False, partition="label_skew",
               partition_skew=0.9, prox_mu=0.01, **ADAM)

    def run():
        client = runner.FederatedClient(cfg, frame=frame, model_config=models.DistilBertConfig(n_layers=1)).setup()
        init = client.model.arena.master.detach().clone()
        runner.run_virtual_clients(client, 2, rounds=2)
        return client, init

    client, init = _single_thread(run)
    assert len(opts) == 4 and len(xs) == 2
    assert torch.equal(opts[0].anchor, init) and torch.equal(opts[1].anchor, init)
    assert torch.equal(opts[2].anchor, xs[0]) and torch.equal(opts[3].anchor, xs[0])
    assert not torch.equal(xs[0], init) and not torch.equal(xs[1], xs[0])
    assert torch.equal(client.server.x, xs[1]) and torch.equal(client.model.arena.master, xs[1])
