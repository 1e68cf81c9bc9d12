"""Single-launch Adam / AdamW over the model's flat parameter arena.

Semantics = ``torch.optim.Adam(model.parameters(), lr=2e-5)`` of the reference
(client1.py:380: betas (0.9, 0.999), eps 1e-8, weight_decay 0, bias-corrected),
with an optional decoupled weight decay (AdamW; BASELINE.json says "AdamW
step" -- identical to Adam at wd = 0).

On GPU the update is the HIP Adam kernel (csrc/kernels/head_optim.hip), which
also refreshes the bf16 compute shadow; the step counter lives on the device so
the update can be replayed inside a HIP graph.  With ``overlap=True`` each
transformer block is updated on a side stream as soon as its
gradients are final, i.e. while the backward of the blocks below it still runs
(Adam is HBM-bound, the backward GEMMs are not), and ``step()`` only updates the
embeddings + head and joins the side stream.  (So between ``backward()`` and
``step()`` the blocks already hold their new weights; pass ``overlap=False`` for
gradient accumulation or to inspect weights there.)  On CPU the same math runs
as flat torch ops.

Measured on MI355X (bs32 x seq128): overlap makes the step SLOWER (3.86 vs
3.51 ms) -- the concurrent Adam blocks take CU slots from the one-round GEMM
grids and HBM bandwidth from LayerNorm/colsum -- so it is off by default.

Fused mode (``fuse_dw=True``, the default; active inside a training step's
``fused_adam_scope``): the encoder's 24 weight matrices (89 % of the dense
parameters) are updated by the weight-gradient GEMMs themselves -- the epilogue
applies Adam to the finished fp32 gradient tile (csrc/kernels/gemm.hip
``adam_epi4``, same arithmetic as the Adam kernel) instead of storing it, so the
gradient never round-trips through HBM and the p/m/v/shadow traffic streams
while other tiles of the grid are still on the MFMAs.  ``step()`` then updates
the rest (embeddings, biases, LayerNorms, head) in one launch over a run table.
The W^T copies the backward's dX GEMMs read are taken before the step, so a
block's later dX GEMMs still see the pre-update weights.  Bitwise identical to
the unfused step (tests/test_fused_adam_gpu.py, tests/test_dw_batch_gpu.py).

With the per-layer grouped dW launches (round 1) it did not pay: each grid runs as
one round, so every tile reached its Adam epilogue at the same time and the ~1.1 GB
of optimizer traffic overlapped nothing (2.39-2.42 vs 2.37-2.38 ms/step,
profiles/r1_ab_fused_adam_fixup.txt).  With all weight gradients of the step in ONE
launch at the end of the backward (RunCtx.dw_batch: ~20 rounds of tiles, no split-K)
the epilogues are staggered behind other tiles' MFMA work, and it does pay:
2.034-2.039 (batched, unfused) vs 1.999-2.000 ms/step (batched + fused), against
2.103 for the per-layer launches (profiles/r2_ab_dw_batch_fused_adam.txt).  On by
default; ``fuse_dw=False`` for the unfused arm.

Weight decay and parameter groups.  ``weight_decay`` follows ``torch.optim.Adam`` (coupled: the
gradient gets ``wd * p``) or, with ``decoupled=True``, ``torch.optim.AdamW`` (``p *= 1 - lr * wd``
before the update).  ``no_decay`` is a sequence of substrings matched against the arena's parameter
names (the HF keys, e.g. ``...sa_layer_norm.weight``, ``...q_lin.bias``); matching parameters form a
second group with decay 0 -- the usual recipe is ``no_decay=("bias", "LayerNorm", "layer_norm")``.
Every launch that applies Adam honours the groups: the run-table launch and the rest blocks of the
all-layer dW launch take a decay per run (runs are split at group boundaries), each fused dW
epilogue takes its matrix's decay, and the qkv bias updated by the dW tiles takes the bias's.  (The
q / k / v parameters of a block are one fused span: they must share a group.)  With
``weight_decay == 0`` nothing changes, bit for bit.

The sparse word-embedding table under weight decay:

1. word table in the no-decay group: the row-flag path is exact as it is (coupled or decoupled);
2. decoupled decay, word table decays: *lazy row decay*, exact to the bit.  A row never touched
   since the moments were reset has m = v = g = 0, so its whole dense AdamW step is
   ``p *= 1 - lr * wd``.  ``row_step`` (int32 per row, ~122 KB) counts the steps whose
   multiplication a row without Adam state has received.  Before the embedding gather of every
   training forward (HIP path) a small launch (``lazy_catchup``; csrc/kernels/head_optim.hip
   adam_lazy_decay_kernel) pays the batch's rows what they are owed -- the number of completed
   steps comes from the device step counter, so it replays inside a captured graph -- and from
   its first gradient a row is updated every step by the row-flag Adam with the real decay.
   The invariant: a row without state that nothing has read since step ``row_step[row]`` is
   ``step - row_step[row]`` multiplications behind.  ``finish()`` settles every row (one launch;
   idempotent; free when no step ran since the last one -- a host-side check) and runs at every
   flush point: ``train_model`` before each ``on_epoch`` callback and before it returns,
   ``state_dict()`` / ``load_state_dict()`` / ``reset_state()`` here, and the model's
   ``state_dict()`` (a hook this optimizer registers).  The other readers of ``arena.master`` --
   FedAvg (parallel/fedavg.py) and the federated runner's exchanges, model sharing and virtual
   clients (fed/runner.py) -- all run after ``train_model`` has returned, i.e. after a flush; code
   that reads ``arena.master`` between the steps of its own loop calls ``finish()`` first;
3. coupled (L2) decay, word table decays: the gradient ``wd * p`` is non-zero for every row, so
   nothing can be skipped -- the dense word gradient and the dense table update, as before;
4. a proximal term (``prox_mu > 0``, below) and the word table decays, coupled or decoupled: a row
   without state decays away from its anchor, so its proximal gradient is non-zero and nothing can
   be skipped either -- the dense path, as in 3 (``dense_word_decay()``).

FedProx (Li et al., 2020).  ``prox_mu > 0`` adds ``mu / 2 * ||w - w_global||^2`` to the local
objective: every gradient gets ``mu * (p - anchor)`` -- taken from the parameter as loaded, before a
decoupled decay multiplies it -- i.e. ``p.grad += mu * (p - p_global)`` followed by
``torch.optim.Adam`` / ``AdamW.step()``.  One scalar for the whole model (biases and LayerNorms
included).  The term lives in the shared element function (csrc/kernels/adam_common.h adam_elem),
so every launch that applies Adam applies it -- the fused weight-gradient epilogues, whose gradient
never exists in memory, included -- and fused and unfused steps stay bitwise equal.  ``anchor`` is
an fp32 copy of the master arena, allocated once (captured graphs keep its address) and re-snapshot
in place only by ``reset_state()``, which the federated runner calls with each round's starting
weights loaded; the same call clears the word table's row flags, hence the invariant *a word row
without Adam state equals its anchor*: its proximal gradient is ``mu * (+0)`` and its whole step
exactly zero, so the row-flag skip (cases 1 and "no decay") stays exact with no lazy machinery.  The
anchor is only read when ``prox_mu != 0`` (+4 B per parameter per step); with ``prox_mu == 0``
nothing changes, bit for bit.  The per-layer fused launches (``linear_dw`` / ``linear_dw2``) refuse
a proximal term as they refuse a schedule.

Learning-rate schedules.  ``schedule="linear"`` is HF ``get_linear_schedule_with_warmup`` (the rate
rises from 0 over ``warmup_steps`` steps, then falls to 0 at ``total_steps``; the first step of a
warmup runs at exactly 0), ``"constant_with_warmup"`` the same ramp and then the base rate.  The
rate of optimizer step t is a formula of ``k = step_offset + t - 1`` that every Adam launch
evaluates on the device from the step counter it already reads (csrc/kernels/adam_common.h
adam_lr_at), so a captured graph -- which holds ``lr`` and the schedule by value -- replays the
whole ramp, and the lazy word-row decay multiplies a row by ``1 - lr_at(s) * wd`` for each missed
step s in order.  ``lr_at(step)`` is the host mirror (float32 arithmetic), used by the CPU path.
``total_steps == 0`` on a non-constant schedule means "resolved by the training loop"
(``train_model`` fills in epochs x batches); ``set_schedule`` changes the numbers only before the
optimizer's first step (or after ``reset_state()``), because captured graphs keep the old ones.
With the default ``schedule="constant"`` nothing changes, bit for bit.

Data-parallel replicas (parallel/dp.py) exchange row flags, which the lazy decay does not cover:
``make_dp_step_fn`` switches a decaying word table to the dense path (``dense_word_decay()``).
"""
from __future__ import annotations

import math
import weakref
from typing import Optional

import numpy as np
import torch

# schedule name -> FdLrSched::kind (csrc/kernels/adam_epi.h)
SCHEDULES = {"constant": 0, "linear": 1, "constant_with_warmup": 2}


def check_schedule(schedule: str, warmup_steps: int, total_steps: int, step_offset: int = 0):
    """Raise ValueError unless the numbers describe a schedule the kernels take (total_steps == 0:
    not resolved yet, see ``ArenaAdam``)."""
    if schedule not in SCHEDULES:
        raise ValueError(f"unknown lr schedule {schedule!r} (one of {', '.join(SCHEDULES)})")
    for name, val in (("warmup_steps", warmup_steps), ("total_steps", total_steps), ("step_offset", step_offset)):
        if int(val) != val or not 0 <= val < 2 ** 30:
            raise ValueError(f"{name} must be an integer in [0, 2^30), got {val}")
    if schedule == "linear" and total_steps > 0 and warmup_steps > total_steps:
        raise ValueError(f"linear schedule: warmup_steps ({warmup_steps}) > total_steps ({total_steps})")


class FusedHyper(list):
    """``fused_args``'s hyper-parameters [lr, b1, b2, eps, wd, decoupled] with the schedule that lr is
    the base rate of (``sched``: None, or the launches' (kind, warmup, total, offset)) and the FedProx
    term (``prox``: None, or (mu, the anchor laid out like the master arena))."""
    sched = None
    prox = None


class ArenaAdam:
    def __init__(self, model, lr: float = 2e-5, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decoupled: bool = False, overlap: bool = False,
                 fuse_dw: bool = True, no_decay=(), schedule: str = "constant", warmup_steps: int = 0,
                 total_steps: int = 0, step_offset: int = 0, warmup_ratio: float = 0.0, prox_mu: float = 0.0):
        if not (math.isfinite(weight_decay) and weight_decay >= 0.0):
            raise ValueError(f"weight_decay must be finite and >= 0, got {weight_decay}")
        if not (math.isfinite(prox_mu) and prox_mu >= 0.0):
            raise ValueError(f"prox_mu must be finite and >= 0, got {prox_mu}")
        self.prox_mu = float(prox_mu)
        self.anchor = None
        if not math.isfinite(lr):
            raise ValueError(f"lr must be finite, got {lr}")
        if not 0.0 <= warmup_ratio <= 1.0:
            raise ValueError(f"warmup_ratio must lie in [0, 1], got {warmup_ratio}")
        check_schedule(schedule, warmup_steps, total_steps, step_offset)
        self.schedule = schedule
        # warmup_ratio: the warmup as a share of total_steps, used while warmup_steps == 0
        self.warmup_steps, self.warmup_ratio = int(warmup_steps), float(warmup_ratio)
        self.total_steps, self.step_offset = int(total_steps), int(step_offset)
        if isinstance(no_decay, str):
            no_decay = no_decay.split(",")
        self.model = model
        self.overlap = overlap
        self.fuse_dw = fuse_dw
        self._run_tables = {}
        self._run_decays = {}
        self.arena = model.arena
        self.lr, self.betas, self.eps = lr, tuple(betas), eps
        self.weight_decay, self.decoupled = weight_decay, decoupled
        self.no_decay = tuple(s.strip() for s in no_decay if s and s.strip())
        self._build_groups()
        prev = getattr(model, "_lazy_decay_opt", None)
        prev = prev() if prev is not None else None
        if prev is not None and prev is not self:
            prev.finish()  # (an earlier optimizer of this model may still owe its rows their decay)
        self._dense_word = False
        if self.word_wd != 0.0 and (not decoupled or self.prox_mu != 0.0):
            # L2 decay reaches every row, and under a proximal term a decaying row without state
            # drifts from its anchor: keep the dense word gradient
            self.dense_word_decay()
        self._alloc()
        if hasattr(model, "word_embedding_span"):
            model._lazy_decay_opt = weakref.ref(self)
            if not getattr(model, "_lazy_decay_hook", False) and hasattr(model, "register_state_dict_pre_hook"):
                model.register_state_dict_pre_hook(_flush_before_state_dict)
                model._lazy_decay_hook = True

    # -------------------------------------------------------------- learning-rate schedule
    def schedule_unresolved(self) -> bool:
        """A non-constant schedule whose total the training loop has yet to fill in."""
        return self.schedule != "constant" and self.total_steps == 0

    def _warmup(self) -> int:
        if self.warmup_steps > 0 or self.warmup_ratio <= 0.0:
            return self.warmup_steps
        return min(self.total_steps, int(math.ceil(self.total_steps * self.warmup_ratio)))

    def set_schedule(self, total_steps=None, warmup_steps=None, step_offset=None):
        """Change the schedule's numbers.  Only before the optimizer's first step since its creation
        or the last ``reset_state()``: captured graphs hold the schedule by value."""
        if self._begun:
            raise RuntimeError("set_schedule inside a step")
        if self.host_step > 0:
            raise RuntimeError("set_schedule after the optimizer has taken a step: captured graphs hold the "
                               "schedule by value (reset_state() first)")
        new = (self.warmup_steps if warmup_steps is None else warmup_steps,
               self.total_steps if total_steps is None else total_steps,
               self.step_offset if step_offset is None else step_offset)
        check_schedule(self.schedule, *new)
        self.warmup_steps, self.total_steps, self.step_offset = (int(x) for x in new)

    def sched_args(self):
        """The ``sched=`` argument of the Adam launches: None (constant) or (kind, warmup, total,
        offset) with ``lr`` as the base rate."""
        if self.schedule == "constant":
            return None
        if self.total_steps == 0:
            raise RuntimeError(f"lr schedule {self.schedule!r}: total_steps is not set (train_model fills it in; "
                               "a hand-written loop calls set_schedule(total_steps=...))")
        return (SCHEDULES[self.schedule], self._warmup(), self.total_steps, self.step_offset)

    def lr_at(self, step: int) -> float:
        """The learning rate of optimizer step ``step`` (1-based): the host mirror of the device
        function (csrc/kernels/adam_common.h adam_lr_at), the same formula in float32 arithmetic."""
        sc = self.sched_args()
        if sc is None:
            return self.lr
        _, warmup, total, offset = sc
        f32 = np.float32
        k = offset + int(step) - 1
        if k < warmup:
            return float(f32(self.lr) * (f32(k) / f32(max(1, warmup))))
        if self.schedule == "constant_with_warmup":
            return float(f32(self.lr))
        return float(f32(self.lr) * (f32(max(0, total - k)) / f32(max(1, total - warmup))))

    # -------------------------------------------------------------- parameter groups
    def _build_groups(self):
        """Decay segments [(start, end, wd)] covering the arena, ascending and merged (a
        parameter's alignment padding -- zeros with zero gradient -- joins its parameter)."""
        A = self.arena
        segs = []
        for name, (off, _shape) in sorted(A.offsets.items(), key=lambda kv: kv[1][0]):
            wd = 0.0 if any(s in name for s in self.no_decay) else float(self.weight_decay)
            if segs and segs[-1][2] == wd:
                continue
            if segs:
                segs[-1][1] = off
            segs.append([off, A.numel, wd])
        if not segs:
            segs = [[0, A.numel, float(self.weight_decay)]]
        segs[0][0] = 0
        segs[-1][1] = A.numel
        self._segs = [tuple(s) for s in segs]
        # groups in effect: the launches take per-run / per-problem decays instead of the scalar
        self.grouped_decay = any(wd != float(self.weight_decay) for _, _, wd in self._segs)
        self.word_wd = 0.0
        if hasattr(self.model, "word_embedding_span"):
            woff, rows, rl = self.model.word_embedding_span()
            self.word_wd = self._span_decay(woff, rows * rl)

    def _span_decay(self, off: int, n: int) -> float:
        """The weight decay of elements [off, off + n): they must lie in one group."""
        wds = {wd for a, b, wd in self._segs if a < off + n and off < b}
        if len(wds) != 1:
            raise ValueError("a span updated by one launch mixes weight-decay groups (q / k / v of a block "
                             "must share a group)")
        return wds.pop()

    def decays_of(self, grads):
        """The weight decay of each arena gradient view's parameters."""
        A = self.arena
        base = A.grad.data_ptr()
        return [self._span_decay((g.data_ptr() - base) // A.grad.element_size(), g.numel()) for g in grads]

    def _split_groups(self, runs):
        """Runs split at group boundaries, and each piece's decay."""
        out, wds = [], []
        for off, n in runs:
            for a, b, wd in self._segs:
                lo, hi = max(off, a), min(off + n, b)
                if lo < hi:
                    out.append((lo, hi - lo))
                    wds.append(wd)
        return out, wds

    # -------------------------------------------------------------- sparse word table under decay
    def dense_word_decay(self):
        """Give up the sparse word-embedding path when the word table decays (coupled decay, or a
        step function whose row flags the lazy decay does not cover: data-parallel replicas)."""
        if self.word_wd == 0.0:
            return
        self.finish()
        self._dense_word = True
        if getattr(self.model, "sparse_word_grad", False):
            self.model.sparse_word_grad = False
            self.model._hip_cache = None

    def lazy_active(self) -> bool:
        """Whether rows of the word table without Adam state decay lazily (case 2 above)."""
        m = self.model
        return (self.word_wd != 0.0 and self.decoupled and not self._dense_word
                and getattr(self, "row_step", None) is not None
                and getattr(m, "impl", None) == "hip" and getattr(m, "sparse_word_grad", False)
                and getattr(m, "emb_ever", None) is not None)

    def _word_views(self):
        A = self.arena
        woff, rows, rl = self.model.word_embedding_span()
        sl = slice(woff, woff + rows * rl)
        return A.master[sl], (A.shadow[sl] if A.shadow is not None else None), rl

    def lazy_catchup(self, ids):
        """Before a training forward gathers rows ``ids``: pay those without Adam state the decay
        of the steps completed so far (the model's HIP forward calls this; replays inside a graph)."""
        if not self.lazy_active():
            return
        from ..ops import kernels as K
        p, sh, rl = self._word_views()
        # (inside a step the counter already counts the running one)
        K.adam_lazy_decay(p, sh, self.row_step, self.model.emb_ever, self.step_t, 1 if self._begun else 0,
                          self.lr, self.word_wd, rl, ids if ids.is_contiguous() else ids.contiguous(),
                          sched=self.sched_args())

    def finish(self):
        """Settle the lazy decay: every word row without Adam state is brought up to the current
        step (one launch).  Idempotent; returns at once when no step ran since the last flush."""
        if not getattr(self, "_lazy_pending", False):
            return
        if not self.lazy_active():
            self._lazy_pending = False
            return
        from ..ops import kernels as K
        p, sh, rl = self._word_views()
        K.adam_lazy_decay(p, sh, self.row_step, self.model.emb_ever, self.step_t, 1 if self._begun else 0,
                          self.lr, self.word_wd, rl, None, sched=self.sched_args())
        self.model.mark_shadow_synced()
        self._lazy_pending = self._begun

    def note_step(self):
        """A step is about to run outside this object's sight (a graph replay): decay is pending."""
        self._lazy_pending = True

    def _alloc(self):
        dev = self.arena.device
        self.m = torch.zeros_like(self.arena.master)
        self.v = torch.zeros_like(self.arena.master)
        # FedProx anchor: the round's starting weights.  Allocated once (captured graphs keep its
        # address) and only ever re-snapshot in place, by reset_state()
        self.anchor = self.arena.master.clone() if self.prox_mu != 0.0 else None
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)
        self.row_step = None  # lazy decay: steps whose decay each word row without state has received
        if dev.type == "cuda" and hasattr(self.model, "word_embedding_span"):
            self.row_step = torch.zeros(self.model.word_embedding_span()[1], dtype=torch.int32, device=dev)
        self._lazy_pending = False
        self.host_step = 0
        self._begun = False
        self._done = []  # (offset, length) spans already updated this step
        use = (self.overlap and dev.type == "cuda" and hasattr(self.model, "layer_span")
               and getattr(self.model, "impl", "hip") == "hip")
        self._side = torch.cuda.Stream(device=dev) if use else None
        if use:
            prev = self.model.layer_grads_hook
            if prev is not None and not isinstance(getattr(prev, "__self__", None), ArenaAdam):
                raise RuntimeError("ArenaAdam(overlap=True) cannot share the backward hook (data-parallel GradSync?)")
            self.model.layer_grads_hook = self._on_layer_grads

    def _begin(self, seed: Optional[torch.Tensor] = None, defer: Optional[list] = None):
        """Advance the device step counter once per step, before the first update launch.
        ``seed``: the model's dropout counter, advanced by the same launch (the model's training
        forward calls this inside a step scope: one tiny kernel instead of two).  ``defer``: append
        the (step, seed) counters to advance there instead of launching -- the caller folds them
        into a launch it makes anyway before anything reads them (the packing kernel)."""
        from ..ops import kernels as K
        self._lazy_pending = True
        if not self._begun:
            if defer is not None:
                defer.append((self.step_t, seed))
            else:
                K.step_inc(self.step_t, seed)
            self.host_step += 1
            self._begun = True
        elif seed is not None:
            if defer is not None:
                defer.append((None, seed))
            else:
                K.step_inc(None, seed)

    def prox_args(self, sl: Optional[slice] = None):
        """The ``prox=`` argument of the Adam launches: None (no proximal term) or (mu, anchor) with
        the anchor of the whole arena, or of its elements ``sl``."""
        if self.prox_mu == 0.0:
            return None
        return (self.prox_mu, self.anchor if sl is None else self.anchor[sl])

    def _hyper(self, wd: float, sl: Optional[slice] = None):
        """This step's hyper-parameters as ``K.adam`` / ``K.adam_rows`` take them, spelled once: the
        positional (lr, b1, b2, eps) and the keywords wd / decoupled / sched / prox, for weight decay
        ``wd`` and the anchor of the whole arena or of its elements ``sl``."""
        b1, b2 = self.betas
        return ((self.lr, b1, b2, self.eps),
                dict(wd=wd, decoupled=self.decoupled, sched=self.sched_args(), prox=self.prox_args(sl)))

    def _update(self, off: int, n: int, sparse: bool):
        from ..ops import kernels as K
        A = self.arena
        sl = slice(off, off + n)
        hp, kw = self._hyper(self._span_decay(off, n) if self.grouped_decay else self.weight_decay, sl)
        if sparse:
            woff, rows, rl = self.model.word_embedding_span()
            kw.update(touched=self.model.emb_ever, now=self.model.emb_now, skip_off=woff - off, skip_rows=rows,
                      row_len=rl)
        K.adam(A.master[sl], A.grad[sl], self.m[sl], self.v[sl], A.shadow[sl], self.step_t, *hp, **kw)

    def _on_layer_grads(self, i: int):
        """Backward hook: block i's gradients are final -> update it on the side stream."""
        if not self.model.training or self._side is None:
            return
        self._begin()
        off, n = self.model.layer_span(i)
        if (off, n) in self._done:
            raise RuntimeError("block gradients finalised twice in one step (gradient accumulation needs "
                               "ArenaAdam(overlap=False))")
        cur = torch.cuda.current_stream(self.arena.device)
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            for o, k in (self._split_groups([(off, n)])[0] if self.grouped_decay else [(off, n)]):
                self._update(o, k, False)
        self._done.append((off, n))

    def can_fuse(self) -> bool:
        """Whether the model's weight-gradient GEMMs may apply this optimizer's step."""
        m = self.model
        # the fused step updates weights inside the backward: safe only when every weight gradient
        # runs in the all-layer launch at the end (after the last dX GEMM that reads W)
        return (self.fuse_dw and not self.overlap and self.arena.device.type == "cuda"
                and getattr(m, "impl", "") == "hip" and getattr(m, "batch_dw", False)
                and getattr(m, "group_dw", False) and getattr(m, "layer_grads_hook", None) is None
                and self.arena.shadow is not None)

    def fused_args(self, grads):
        """(state tensors, hyper-parameters) for a weight-gradient GEMM that applies Adam to
        ``grads`` (arena grad views) in its epilogue; those spans are skipped by ``step()``.  The
        hyper-parameters carry the schedule (``FusedHyper.sched``): the all-layer launch passes it on
        (ops/kernels.py linear_dw_batch), the per-layer launches, which take none, refuse it."""
        from ..ops import kernels as K  # noqa: F401  (extension must be present)
        self._begin()
        A = self.arena
        base = A.grad.data_ptr()
        st = []
        for g in grads:
            off = (g.data_ptr() - base) // A.grad.element_size()
            n = g.numel()
            if not (0 <= off and off + n <= A.numel) or not g.is_contiguous():
                raise ValueError("fused Adam: gradient is not a contiguous arena view")
            st += [A.master[off:off + n], self.m[off:off + n], self.v[off:off + n], A.shadow[off:off + n]]
            self._done.append((off, n))
        st.append(self.step_t)
        pos, kw = self._hyper(self.weight_decay)
        hp = FusedHyper([*pos, kw["wd"], 1.0 if kw["decoupled"] else 0.0])
        hp.sched, hp.prox = kw["sched"], kw["prox"]
        return st, hp

    def _runs_table(self, runs):
        """Cached device run table for ``runs`` (built during the eager warm-up steps, so a
        graph capture never needs a host->device copy)."""
        key = tuple(runs)
        t = self._run_tables.get(key)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                return None
            from ..ops import kernels as K
            t = K.adam_runs(runs, self.arena.device)
            self._run_tables[key] = t
            if self.grouped_decay:
                self._run_decays[key] = K.adam_run_decay([self._span_decay(o, n) for o, n in runs],
                                                         self.arena.device)
        return t

    def _runs_decay(self, runs):
        """The per-run decays that go with ``_runs_table(runs)`` (None: one group)."""
        return self._run_decays.get(tuple(runs))

    def rest_decay_args(self):
        """Keyword arguments of ``gemm_dw_batch`` for the decays of the rest ``rest_args`` returned."""
        kw = {}
        rd = self._runs_decay(self._rest_key) if self.grouped_decay else None
        if rd is not None:
            kw["rest_wd"], kw["rest_wd_host"] = rd
        if self.word_wd != 0.0:
            kw["word_wd"] = self.word_wd
        return kw

    def reset_state(self):
        """FedAvg rounds restart the moments (the reference re-creates Adam each run)."""
        self.finish()
        if self.row_step is not None:
            self.row_step.zero_()
        self.m.zero_()
        self.v.zero_()
        self.step_t.zero_()
        self.host_step = 0
        self._done, self._begun = [], False
        self._rest_in_launch = False
        if getattr(self.model, "emb_ever", None) is not None:
            self.model.emb_ever.zero_()
        if self.anchor is not None:
            # the round's starting weights, in place (after finish(): the settled master), and in
            # the same call that clears the row flags: a word row without state equals its anchor
            self.anchor.copy_(self.arena.master)

    def zero_grad(self, set_to_none: bool = False):
        self.model.zero_grad()

    def mark_done(self, grads):
        """Arena gradient views that a launch other than ``step()`` updates this step (the qkv
        biases, updated by the all-layer weight-gradient tiles that sum their gradient)."""
        self._begin()
        A = self.arena
        base = A.grad.data_ptr()
        for g in grads:
            off = (g.data_ptr() - base) // A.grad.element_size()
            if not (0 <= off and off + g.numel() <= A.numel) or not g.is_contiguous():
                raise ValueError("mark_done: not a contiguous arena gradient view")
            self._done.append((off, g.numel()))

    def _sparse_words(self) -> bool:
        # Only the HIP path leaves a sparse word gradient (and sets the emb_now / emb_ever row
        # flags, in its embedding backward): the torch path's autograd writes the dense table
        # and sets no flag, so the row-flag Adam would skip every word row there.  (Round 3's
        # "HIP learns faster than fp32" loss-curve bias was exactly that: the fp32 reference
        # arm on the GPU never updated its word embeddings -- results/numerics_r4/.)
        hip_sparse = getattr(self.model, "impl", None) == "hip" and getattr(self.model, "sparse_word_grad", False)
        # exact when the word table does not decay; with decoupled decay the rows without state
        # decay lazily (lazy_catchup / finish); coupled decay needs the dense table
        sparse = (hip_sparse and (self.word_wd == 0.0 or self.lazy_active())
                  and getattr(self.model, "emb_ever", None) is not None)
        if hip_sparse and not sparse and getattr(self.model, "emb_now", None) is not None:
            raise RuntimeError("sparse word-embedding grads with a decaying word table need decoupled "
                               "weight decay (set model.sparse_word_grad = False otherwise)")
        return sparse

    def _rest_runs(self, sparse: bool):
        """(runs, rest): every element span not updated yet this step, and -- with the sparse word
        table -- the same minus that table (which the row-flag Adam takes)."""
        A = self.arena
        done = sorted(self._done)
        pos, runs = 0, []
        for off, n in done:
            if off > pos:
                runs.append((pos, off - pos))
            pos = max(pos, off + n)
        if pos < A.numel:
            runs.append((pos, A.numel - pos))
        if self.grouped_decay:
            runs, _ = self._split_groups(runs)
        if not sparse:
            return runs, None
        woff, rows, rl = self.model.word_embedding_span()
        wend = woff + rows * rl
        rest = []
        for off, n in runs:
            a, b = off, off + n
            if b <= woff or a >= wend:
                rest.append((a, n))
                continue
            if not (a <= woff and wend <= b):
                raise RuntimeError("the word-embedding table must lie inside one Adam run")
            if woff > a:
                rest.append((a, woff - a))
            if b > wend:
                rest.append((wend, b - wend))
        return runs, rest

    def rest_args(self):
        """The rest of this step's update for the all-layer weight-gradient launch to run beside its
        last tiles (csrc/kernels/gemm.hip dwb_rest; FD_ADAM_IN_DW=0: ``step()`` launches it):
        (tensors, ints) for ``gemm_dw_batch(rest=, rest_i=)``, or None when it cannot (no cached
        run table during a capture, a dense word table, ...).  Call after every other span of the
        step is marked done; ``step()`` then only finishes the bookkeeping."""
        from ..ops import kernels as K
        A = self.arena
        if not (K.ADAM_IN_DW and A.master.is_cuda and self._side is None and A.shadow is not None):
            return None
        self._begin()
        sparse = self._sparse_words()
        if not sparse:
            return None
        _, rest = self._rest_runs(True)
        if not rest:
            return None
        table = self._runs_table(rest)
        if table is None:
            return None
        woff, rows, rl = self.model.word_embedding_span()
        tab, total4, _ = table
        self._rest_key = tuple(rest)
        self._rest_in_launch = True
        return ([A.master, A.grad, self.m, self.v, A.shadow, tab, self.model.emb_ever, self.model.emb_now],
                [total4, woff, rows, rl])

    @torch.no_grad()
    def step(self):
        A = self.arena
        if A.master.device != self.m.device:
            self._alloc()
        b1, b2 = self.betas
        self.sched_args()  # (raises while a schedule's total is unresolved)
        if A.master.is_cuda:
            self._begin()
            if getattr(self, "_rest_in_launch", False):
                # the all-layer weight-gradient launch already ran the rest (rest_args)
                self._rest_in_launch = False
                if self._side is not None:
                    torch.cuda.current_stream(A.device).wait_stream(self._side)
                self.model.mark_shadow_synced()
                self._done = []
                self._begun = False
                return
            sparse = self._sparse_words()
            # everything not already updated by the per-block hook, in contiguous runs
            runs, rest = self._rest_runs(sparse)
            woff = self.model.word_embedding_span()[0] if sparse else -1
            table = self._runs_table(runs) if len(runs) > 1 else None
            if table is not None and sparse:
                # the word-embedding table by its row flags (one wave per 64 rows: only rows with
                # Adam state are touched), everything else left in one run-table launch
                from ..ops import kernels as K
                _, rows, rl = self.model.word_embedding_span()
                wend = woff + rows * rl
                sl = slice(woff, wend)
                hp, kw = self._hyper(self.word_wd, sl)
                K.adam_rows(A.master[sl], A.grad[sl], self.m[sl], self.v[sl], A.shadow[sl], self.step_t, *hp,
                            self.model.emb_ever, self.model.emb_now, rl, **kw)
                rest_table = self._runs_table(rest) if len(rest) > 1 else None
                if rest_table is not None:
                    hp, kw = self._hyper(self.weight_decay)
                    K.adam(A.master, A.grad, self.m, self.v, A.shadow, self.step_t, *hp, runs=rest_table,
                           run_decay=self._runs_decay(rest), **kw)
                else:
                    for off, n in rest:
                        self._update(off, n, False)
            elif table is not None:  # everything left (fused-GEMM spans excluded) in one launch
                from ..ops import kernels as K
                hp, kw = self._hyper(self.weight_decay)
                K.adam(A.master, A.grad, self.m, self.v, A.shadow, self.step_t, *hp, runs=table,
                       run_decay=self._runs_decay(runs), **kw)
            else:
                for off, n in runs:
                    self._update(off, n, sparse and off <= woff < off + n)
            if self._side is not None:
                torch.cuda.current_stream(A.device).wait_stream(self._side)
            self.model.mark_shadow_synced()
            self._done = []
            self._begun = False
            return
        self.host_step += 1
        t = self.host_step
        self.step_t += 1
        lr = self.lr_at(t)
        p, g = A.master, A.grad
        if self.prox_mu != 0.0:  # FedProx: from p as it is, before a decoupled decay multiplies it
            g = g + self.prox_mu * (p - self.anchor)
        if self.weight_decay and self.grouped_decay:  # one group per segment, as torch.optim's param groups
            if not self.decoupled:
                g = g.clone()
            for a, b, wd in self._segs:
                if wd == 0.0:
                    continue
                if self.decoupled:
                    p[a:b].mul_(1 - lr * wd)
                else:
                    g[a:b] += wd * p[a:b]
        elif self.weight_decay:
            if self.decoupled:
                p.mul_(1 - lr * self.weight_decay)
            else:
                g = g + self.weight_decay * p
        self.m.mul_(b1).add_(g, alpha=1 - b1)
        self.v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1 = 1 - b1 ** t
        bc2 = 1 - b2 ** t
        denom = (self.v.sqrt() / math.sqrt(bc2)).add_(self.eps)
        p.addcdiv_(self.m, denom, value=-lr / bc1)
        self.model.mark_shadow_synced()

    def state_dict(self):
        self.finish()
        sd = {"m": self.m.cpu(), "v": self.v.cpu(), "step": int(self.step_t.item()),
              "lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
              "decoupled": self.decoupled}
        if self.schedule != "constant":  # (the constant schedule keeps the dictionary's keys as they were)
            sd["schedule"] = {"name": self.schedule, "warmup_steps": self.warmup_steps,
                              "warmup_ratio": self.warmup_ratio, "total_steps": self.total_steps,
                              "step_offset": self.step_offset}
        if self.prox_mu != 0.0:  # (the anchor is not saved: a resumed job restarts at a round boundary)
            sd["prox_mu"] = self.prox_mu
        return sd

    def load_state_dict(self, sd):
        self.finish()  # (before every row counts as having state)
        sch = sd.get("schedule")
        if sch is not None:  # resume at the saved point of the ramp
            check_schedule(sch["name"], sch["warmup_steps"], sch["total_steps"], sch["step_offset"])
            self.schedule = sch["name"]
            self.warmup_steps, self.warmup_ratio = int(sch["warmup_steps"]), float(sch.get("warmup_ratio", 0.0))
            self.total_steps, self.step_offset = int(sch["total_steps"]), int(sch["step_offset"])
        if getattr(self.model, "emb_ever", None) is not None:
            self.model.emb_ever.fill_(1)  # unknown history: treat every row as having state
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.step_t.fill_(int(sd["step"]))
        self.host_step = int(sd["step"])


def _flush_before_state_dict(module, *_args, **_kw):
    """``state_dict`` pre-hook of a model whose optimizer decays word rows lazily."""
    ref = getattr(module, "_lazy_decay_opt", None)
    opt = ref() if ref is not None else None
    if opt is not None:
        opt.finish()
