"""AdamW on the CPU (torch path): ArenaAdam's weight decay and no-decay parameter group against
torch.optim, the --no-decay / FEDDDOS_NO_DECAY plumbing, and the data-parallel fallback."""
import argparse

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.config import FedConfig
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import ArenaAdam
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.fed.runner import (
    make_optimizer)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier, DistilBertConfig)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.parallel.dp import (
    make_dp_step_fn)

HF_NO_DECAY = ("bias", "LayerNorm", "layer_norm")
WORD = "distilbert.embeddings.word_embeddings.weight"


def small(layers=1, seed=0):
    return DDoSClassifier(config=DistilBertConfig(n_layers=layers), seed=seed)


def batch(B=4, S=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(999, 2000, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1:, S // 2:] = 0
    ids = ids * mask
    ids[:, 0] = 101
    return ids, mask, torch.randint(0, 2, (B,), generator=g)


def _is_no_decay(name):
    return any(s in name for s in HF_NO_DECAY)


def _torch_optimizer(model, kind):
    if kind == "adam":
        return torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.01)
    if kind == "adamw":
        return torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    named = list(model.named_parameters())
    decay = [p for n, p in named if not _is_no_decay(n)]
    plain = [p for n, p in named if _is_no_decay(n)]
    assert decay and plain
    return torch.optim.AdamW([{"params": decay, "weight_decay": 0.01}, {"params": plain, "weight_decay": 0.0}],
                             lr=1e-3)


def _train(model, opt, arena_opt):
    ids, mask, y = batch()
    model.train()
    for step in range(3):
        model.torch_counter = step
        if arena_opt:
            opt.zero_grad()
        else:
            opt.zero_grad(set_to_none=False)
            model.zero_grad()
        loss, _ = model.forward_loss(ids, mask, y)
        loss.backward()
        opt.step()
    return {k: v.clone() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def arena_runs():
    """ArenaAdam after 3 steps: coupled, decoupled (one group), decoupled with the HF no-decay group."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)  # (as tests/test_model_cpu.py: the GEMM reductions split by thread count)
    try:
        out = {}
        for kind, kw in (("adam", dict(decoupled=False)), ("adamw", dict(decoupled=True)),
                         ("groups", dict(decoupled=True, no_decay=HF_NO_DECAY))):
            m = small(seed=3)
            out[kind] = _train(m, ArenaAdam(m, lr=1e-3, weight_decay=0.01, **kw), True)
        return out
    finally:
        torch.set_num_threads(nthreads)


@pytest.mark.parametrize("kind", ["adam", "adamw", "groups"])
def test_arena_adam_weight_decay_matches_torch(arena_runs, kind):
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m = small(seed=3)
        ref = _train(m, _torch_optimizer(m, kind), False)
    finally:
        torch.set_num_threads(nthreads)
    got = arena_runs[kind]
    assert list(got) == list(ref)
    for k in ref:
        if k.endswith("k_lin.bias"):
            # softmax is invariant to the key bias: its true gradient is 0 and Adam amplifies
            # round-off noise (|g| ~ 1e-10 << eps), so both runs move it by noise only.
            continue
        assert torch.allclose(got[k], ref[k], atol=1e-6, rtol=1e-5), k


def test_no_decay_group_is_not_decayed(arena_runs):
    """The no-decay parameters of the grouped run differ from the all-decay run (3 steps of
    p *= 1 - 1e-5 move a LayerNorm gain of ~1 by ~3e-5)."""
    allp, grp = arena_runs["adamw"], arena_runs["groups"]
    differ = [k for k in allp if _is_no_decay(k) and not k.endswith("k_lin.bias")
              and not torch.equal(allp[k], grp[k])]
    assert any("layer_norm.weight" in k for k in differ) and any("LayerNorm.weight" in k for k in differ)
    k = "distilbert.transformer.layer.0.sa_layer_norm.weight"
    gap = (grp[k] - allp[k]).abs().max().item()
    assert 2e-5 < gap < 4e-5, gap  # |p| ~ 1: 1 - (1 - 1e-5)^3


def test_group_segments_and_validation():
    m = small()
    opt = ArenaAdam(m, weight_decay=0.01, decoupled=True, no_decay=HF_NO_DECAY)
    A = m.arena
    names = list(A.names())
    wds = dict(zip(names, opt.decays_of([A.gview(n) for n in names])))
    assert len(names) == 22  # embeddings (4) + one block (16) + head (2)
    for n, wd in wds.items():
        assert wd == (0.0 if _is_no_decay(n) else 0.01), n
    assert opt.grouped_decay and opt.word_wd == 0.01
    # runs are split where the decay changes, and every piece lies in one group
    pieces, piece_wd = opt._split_groups([(0, A.numel)])
    assert sum(n for _, n in pieces) == A.numel and len(pieces) > 2
    assert all(opt._span_decay(o, n) == wd for (o, n), wd in zip(pieces, piece_wd))
    # one group: the scalar path, as before
    assert not ArenaAdam(small(), weight_decay=0.01, decoupled=True).grouped_decay
    assert not ArenaAdam(small(), no_decay=HF_NO_DECAY).grouped_decay  # weight_decay == 0: nothing to group
    # a fused span (q / k / v of a block) must lie in one group
    bad = ArenaAdam(small(), weight_decay=0.01, decoupled=True, no_decay=("q_lin",))
    pre = "distilbert.transformer.layer.0.attention."
    with pytest.raises(ValueError, match="groups"):
        bad.decays_of([A.span([pre + "q_lin.weight", pre + "k_lin.weight", pre + "v_lin.weight"], "grad")])
    with pytest.raises(ValueError):
        ArenaAdam(small(), weight_decay=-0.01)
    with pytest.raises(ValueError):
        ArenaAdam(small(), weight_decay=float("nan"))


def test_no_decay_reaches_the_runner_optimizer(monkeypatch):
    parser = FedConfig.add_cli(argparse.ArgumentParser())
    ns = parser.parse_args(["--weight-decay", "0.01", "--decoupled-weight-decay", "true",
                            "--no-decay", "bias,LayerNorm,layer_norm"])
    cfg = FedConfig.from_args(ns)
    assert cfg.no_decay == "bias,LayerNorm,layer_norm"
    m = small()
    opt = make_optimizer(m, cfg)
    assert opt.no_decay == HF_NO_DECAY and opt.weight_decay == 0.01 and opt.decoupled
    A = m.arena
    pre = "distilbert.transformer.layer.0."
    assert opt.decays_of([A.gview(pre + "attention.q_lin.bias"), A.gview(pre + "sa_layer_norm.weight"),
                          A.gview(pre + "ffn.lin1.weight"), A.gview(WORD)]) == [0.0, 0.0, 0.01, 0.01]

    monkeypatch.setenv("FEDDDOS_NO_DECAY", "bias, word_embeddings")
    monkeypatch.setenv("FEDDDOS_WEIGHT_DECAY", "0.05")
    cfg = FedConfig.from_env()
    opt = make_optimizer(small(), cfg)
    assert opt.no_decay == ("bias", "word_embeddings") and opt.weight_decay == 0.05 and not opt.decoupled
    assert opt.word_wd == 0.0
    assert make_optimizer(small(), FedConfig()).no_decay == ()


def test_sparse_word_table_choice_and_dp_fallback():
    """Which optimizers keep the sparse word-embedding path, and the data-parallel step function's
    fallback to the dense table when the word table decays (its exchanged row flags are outside
    the lazy row decay)."""
    sync = object()  # (only the step itself uses it)
    # coupled decay of the word table: dense from the start
    m = small()
    ArenaAdam(m, weight_decay=0.01)
    assert m.sparse_word_grad is False
    # word table in the no-decay group: sparse, coupled or decoupled, data-parallel too
    for dec in (False, True):
        m = small()
        opt = ArenaAdam(m, weight_decay=0.01, decoupled=dec, no_decay=("word_embeddings",))
        assert m.sparse_word_grad is True and opt.word_wd == 0.0
        make_dp_step_fn(m, opt, sync)
        assert m.sparse_word_grad is True
    # decoupled decay of the word table: sparse (lazy row decay) for a single-GPU step ...
    m = small()
    opt = ArenaAdam(m, weight_decay=0.01, decoupled=True, no_decay=HF_NO_DECAY)
    assert m.sparse_word_grad is True and opt.word_wd == 0.01
    # ... and dense once a data-parallel step function is built on it
    make_dp_step_fn(m, opt, sync)
    assert m.sparse_word_grad is False and not opt.lazy_active()
    # no weight decay: untouched
    m = small()
    opt = ArenaAdam(m)
    make_dp_step_fn(m, opt, sync)
    assert m.sparse_word_grad is True
