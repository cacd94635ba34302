"""TableAdam: the reference's dense Adam + L2 over the tables of `FeatureEmbedding` and `LinearModel` at touched-rows cost.

The reference trains every table as a dense parameter: `torch.optim.Adam` over dense gradients, with the regulariser
`l2 * sum(p^2)` added to the loss, so EVERY row moves on EVERY step (a row nobody gathered still sees the gradient 2 l2 p, and
its moments decay).  Un-adopted, the two modules give exactly that to any torch optimizer - through a zero-filled gradient
buffer of the tables' size and an optimizer sweep over three such buffers per step.  The arithmetic of a cheaper step has
been in csrc/embed_adam.hip since the engine was written (the sort, the ordered segment sums with Adam on the touched rows, the
lazy replay and flush: bit for bit the every-row streaming step); this class makes it reachable from the two modules.

    opt = TableAdam([fe, lin], lr=1e-3, l2_reg_embedding=1e-5, l2_reg_linear=1e-5)
    emb, dense = fe(X); logit = lin(X); loss = ...; loss.backward()
    opt.step()                      # the tables (and LinearModel.weight); the head keeps its own torch optimizer

An adopted module changes in three places (layers.py): its forward first brings the rows of the batch to the completed step
count `t` (lazy form; also under no_grad and in eval(), so what a forward reads is always current); its backward builds no
[rows, D] buffer and leaves every table's `.grad` None - it hands (sorted_rows, src, gemb) to the optimizer; and `step()` runs
satrans_embed_adam_touched on those rows.  Laziness only postpones a row's regulariser-only steps until the row is next
gathered or until a flush; `flush()` brings every row to `t`, and runs by itself every `flush_every` steps, before the
`state_dict()` of an adopted module and before `opt.state_dict()`.  Reading `embedding_dict[...].weight` directly between steps
sees the postponed rows as they were left: call `opt.flush()` first.

`lazy=False` is the streaming form (satrans_embed_mark_touched, satrans_embed_adam_untouched, satrans_embed_adam_touched every
step): the same bits, a sweep per step; the tests hold the lazy form against it.  The 1-wide tables of LinearModel step by one
satrans_adam_flat(l2_reg_linear) over a gradient buffer the optimizer owns (`linear_lazy=False`, the default - DESIGN.md
§3.20) or by the lazy 1-wide kernels (`linear_lazy=True`: satrans_embed1_lazy_replay / _adam_rows / _lazy_flush, the same
bits).  `LinearModel.weight` takes satrans_adam_flat in the exact arithmetic, as the engine's flat parameters do.

The learning rate is read from `param_groups[0]["lr"]` at every step, so torch.optim.lr_scheduler works; a rate change needs
no flush, because the replay reads each step's constants from a per-step table (`StepTable`, built as PathEngine._table builds
its own).  betas and eps are fixed at construction.  Only the gradient of the regulariser is applied; its VALUE is computed on
request: `track_regularizer=True` adds the partial sums the touched, untouched, replay and flush kernels write (l2 * p^2 at the
pre-step values) into one device double, one satrans_sum_f64 launch after each of them - the replay and the flush then run as
satrans_embed_lazy_replay_reg64 / satrans_embed_lazy_flush_reg64, the same tables and moments with every replayed p^2 formed in
double as the step kernels form it, so that the lazy and the streaming totals are the same terms in another grouping - and, for the 1-wide arena and
`LinearModel.weight`, whose satrans_adam_flat step writes none - l2 * sum(p^2) by a torch reduction, which costs one more read
of the 1-wide arena per step (`regularization_sum()`).  Off (the default), the optimizer runs the launches it always ran.
Not built: gradient accumulation (a second backward before step() raises), optimizers other than Adam, several
ranks, weight_decay / amsgrad / maximize, a second param group."""
from __future__ import annotations

import ctypes as C
import math
from typing import List

import numpy as np
import torch

from . import native as N

ARITH = {"exact": N.ADAM_EXACT, "fast": N.ADAM_FAST}


class StepTable:
    """Per-step Adam constants for the replay kernels, host side: row s = (fp32(lr_s / (1 - beta1^s)), 1 / fp32(sqrt(1 - beta2^s)))
    as doubles, row 0 = (0, 1) - exactly what `hparams` hands the step kernels at step s (the same Python arithmetic for the
    powers; the division and the fp32 rounding are IEEE operations in numpy as in Python).  lr_s is the rate step s was taken
    with: `note(s, lr)` writes the rows from s on, so the rows of earlier, possibly still postponed, steps keep their rate."""

    def __init__(self, betas, cap: int = 4096):
        self.betas = (float(betas[0]), float(betas[1]))
        self.lr = None                # the rate the rows from the last change on are filled with
        self.rows = np.zeros((0, 2), dtype=np.float64)
        self._bc1 = np.zeros(0, dtype=np.float64)
        self._dev = None
        self._dirty = None            # first row the device copy does not have yet
        self._grow(cap)

    def _grow(self, cap: int) -> None:
        old = self.rows.shape[0]
        if cap <= old:
            return
        b1, b2 = self.betas
        f32 = lambda x: float(np.float32(x))      # noqa: E731  (the value the fp32 kernels, and torch's fp32 step, see)
        bc1 = np.array([1.0 if s == 0 else 1.0 - b1 ** s for s in range(old, cap)], dtype=np.float64)
        col1 = np.array([1.0 if s == 0 else 1.0 / f32(math.sqrt(1.0 - b2 ** s)) for s in range(old, cap)], dtype=np.float64)
        col0 = np.zeros(cap - old, dtype=np.float64) if self.lr is None else np.float32(self.lr / bc1).astype(np.float64)
        if old == 0:
            col0[0] = 0.0
        self._bc1 = np.concatenate([self._bc1, bc1])
        self.rows = np.concatenate([self.rows, np.stack([col0, col1], axis=1)], axis=0)
        self._dev = None

    def note(self, s: int, lr: float) -> None:
        """Step s (and, until further notice, every later one) is taken with the rate `lr`."""
        if s >= self.rows.shape[0]:
            self._grow(2 * (s + 1))
        if self.lr is None or lr != self.lr:
            self.lr = lr
            self.rows[s:, 0] = np.float32(lr / self._bc1[s:]).astype(np.float64)
            self._dirty = s if self._dirty is None else min(self._dirty, s)

    def device(self, upto: int, dev) -> torch.Tensor:
        """[>= upto + 1, 2] fp64 on `dev`; only the rows a rate change rewrote travel again."""
        if upto >= self.rows.shape[0]:
            self._grow(2 * (upto + 1))
        if self._dev is None or self._dev.device != torch.device(dev):
            self._dev = torch.from_numpy(self.rows).to(dev).contiguous()
        elif self._dirty is not None:
            self._dev[self._dirty:].copy_(torch.from_numpy(self.rows[self._dirty:]))
        self._dirty = None
        return self._dev


class _Adopted:
    """One adopted module: its moments, the last step of every row, and the gradient its backward handed over."""

    def __init__(self, opt, mod, kind: str, l2: float):
        self.opt, self.mod, self.kind, self.l2 = opt, mod, kind, float(l2)
        arena = mod.arena
        weight = getattr(mod, "weight", None) if kind == "linear" else None
        self.dev = arena.device if arena is not None else weight.device
        self.m = self.v = self.last = self.g = self.wm = self.wv = None
        if arena is not None:
            self.m, self.v = torch.zeros_like(arena), torch.zeros_like(arena)
            self.last = torch.zeros(arena.shape[0], dtype=torch.int32, device=self.dev)
            if kind == "linear":
                self.g = torch.zeros_like(arena)      # the gradient buffer of the 1-wide tables
        if weight is not None:
            self.wm, self.wv = torch.zeros_like(weight.data), torch.zeros_like(weight.data)
        self.pending = None
        self._ws = {}

    # the lazy form of this module's tables
    @property
    def lazy(self) -> bool:
        return self.m is not None and (self.opt.lazy if self.kind == "embedding" else self.opt.linear_lazy)

    def check_device(self) -> None:
        p = self.mod.arena if self.mod.arena is not None else self.mod.weight
        if p.device != self.dev:
            raise RuntimeError(f"TableAdam: {type(self.mod).__name__} was adopted on {self.dev} and now lies on {p.device}; the "
                               f"optimizer state does not follow a module to another device (move it back, or build a new optimizer)")

    def arena(self) -> torch.Tensor:
        """The arena as it is NOW (`_tables()` may rebind it: no pointer of it is kept between calls)."""
        self.mod._tables()
        return self.mod.arena

    def drop(self) -> None:
        if self.pending is not None and self.g is not None and self.lazy:
            self.g.zero_()            # (the lazy 1-wide step is what clears the rows a backward wrote)
        self.pending = None

    def scratch(self, name, size, dtype, zero=False):
        key = (name, int(size), dtype)
        if key not in self._ws:
            self._ws = {k: t for k, t in self._ws.items() if k[0] != name}
            self._ws[key] = (torch.zeros if zero else torch.empty)(max(int(size), 1), dtype=dtype, device=self.dev)
        return self._ws[key]

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def replay(self, sorted_rows, n: int) -> None:
        """FeatureEmbedding, lazy: the postponed steps of exactly these rows, up to the completed step count."""
        opt = self.opt
        if opt._since_flush == 0:      # every row stands at t
            return
        lib, arena = N.lib(), self.arena()
        D = arena.shape[1]
        h = opt.hparams(self.l2, opt.arith)
        reg = self.scratch("lazy_reg", lib.satrans_embed_lazy_reg_partials(n, D), torch.float64, zero=True)
        call = lib.satrans_embed_lazy_replay_reg64 if opt.track_regularizer else lib.satrans_embed_lazy_replay
        N.check(call(arena.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.last.data_ptr(), D, sorted_rows.data_ptr(), n, opt.t,
                     opt.table(self.dev).data_ptr(), C.byref(h), reg.data_ptr(), N.stream_handle(self.dev)), "satrans_embed_lazy_replay")
        opt._add_reg(reg, (n * D + 255) // 256, self.dev)      # (the slots this call wrote; the rest of the buffer is the flush's)

    def replay_linear(self, d) -> None:
        """LinearModel, lazy: every slot row of the batch behind the descriptor `d`, before satrans_linear_fwd reads it."""
        opt = self.opt
        if opt._since_flush == 0:
            return
        lib, arena = N.lib(), self.arena()
        h = opt.hparams(self.l2, opt.arith)
        N.check(lib.satrans_embed1_lazy_replay(arena.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.last.data_ptr(),
                                               arena.shape[0], None, 0, d.fields, d.F, d.R, d.X, d.id_dtype, d.x_stride, d.B, opt.t,
                                               opt.table(self.dev).data_ptr(), C.byref(h), N.stream_handle(self.dev)),
                "satrans_embed1_lazy_replay")

    # ---- backward --------------------------------------------------------------------------------------------------------------
    def refuse_second(self) -> None:
        if self.pending is not None:
            self.drop()
            raise RuntimeError(f"TableAdam: a second backward through {type(self.mod).__name__} before step(): gradient "
                               f"accumulation is not built (both gradients are dropped; run forward and backward again)")

    def take(self, sorted_rows, src, grad, n: int, fwd_t: int) -> None:
        self.pending = (sorted_rows, src, grad, n, fwd_t)

    # ---- step ------------------------------------------------------------------------------------------------------------------
    def step(self, t: int) -> None:
        opt, lib, st = self.opt, N.lib(), N.stream_handle(self.dev)
        sorted_rows, src, grad, n, _ = self.pending
        self.pending = None
        if self.kind == "embedding":
            arena = self.arena()
            total, D = arena.shape
            h = opt.hparams(self.l2, opt.arith)
            part = self.scratch("partial", lib.satrans_embed_partial_ws_floats(n, D), torch.float32)
            # (tracked: zero-filled once, because the lazy form never writes the slots of the streaming kernel)
            reg = self.scratch("reg", lib.satrans_embed_reg_partials(total, n, D), torch.float64, zero=opt.track_regularizer)
            if not opt.lazy:
                bitmap = self.scratch("touched", (total + 31) // 32, torch.int32)
                N.check(lib.satrans_embed_mark_touched(sorted_rows.data_ptr(), n, total, bitmap.data_ptr(), st),
                        "satrans_embed_mark_touched")
                N.check(lib.satrans_embed_adam_untouched(arena.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), 0, total, D,
                                                         bitmap.data_ptr(), C.byref(h), reg.data_ptr(), 0, st),
                        "satrans_embed_adam_untouched")
            N.check(lib.satrans_embed_adam_touched(arena.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), D, sorted_rows.data_ptr(),
                                                   src.data_ptr(), n, grad.data_ptr(), part.data_ptr(), C.byref(h), reg.data_ptr(),
                                                   self.last.data_ptr() if opt.lazy else None, t if opt.lazy else 0, st),
                    "satrans_embed_adam_touched")
            opt._add_reg(reg, reg.numel(), self.dev)
            return
        if self.m is not None:
            arena = self.arena()
            h = opt.hparams(self.l2, opt.arith)
            opt._add_reg_of(arena, self.l2)
            if self.lazy:
                N.check(lib.satrans_embed1_adam_rows(arena.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.last.data_ptr(),
                                                     self.g.data_ptr(), arena.shape[0], sorted_rows.data_ptr(), n, C.byref(h), t, st),
                        "satrans_embed1_adam_rows")
            else:
                N.check(lib.satrans_adam_flat(arena.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                              arena.numel(), C.byref(h), st), "satrans_adam_flat")
        if self.wm is not None:
            w = self.mod.weight.data
            h = opt.hparams(self.l2, "exact")
            opt._add_reg_of(w, self.l2)
            N.check(lib.satrans_adam_flat(N.ptr(w), grad.data_ptr(), self.wm.data_ptr(), self.wv.data_ptr(), w.numel(), C.byref(h),
                                          st), "satrans_adam_flat")

    def flush(self, t: int) -> None:
        if not self.lazy:
            return
        opt, lib, st = self.opt, N.lib(), N.stream_handle(self.dev)
        arena = self.arena()
        h = opt.hparams(self.l2, opt.arith)
        table = opt.table(self.dev)
        if self.kind == "embedding":
            reg = self.scratch("flush_reg", 4096, torch.float64)
            call = lib.satrans_embed_lazy_flush_reg64 if opt.track_regularizer else lib.satrans_embed_lazy_flush
            N.check(call(arena.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.last.data_ptr(), arena.shape[0], arena.shape[1],
                         t, table.data_ptr(), C.byref(h), 0, reg.data_ptr(), st), "satrans_embed_lazy_flush")
            opt._add_reg(reg, reg.numel(), self.dev)
        else:
            N.check(lib.satrans_embed1_lazy_flush(arena.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.last.data_ptr(),
                                                  arena.shape[0], t, table.data_ptr(), C.byref(h), st), "satrans_embed1_lazy_flush")

    # ---- state -----------------------------------------------------------------------------------------------------------------
    def moments(self):
        """state_dict key of the module -> (exp_avg, exp_avg_sq), views of this module's buffers."""
        out = {}
        if self.m is not None:
            for name in self.mod._layout.names:
                lo, cnt = self.mod._layout.table_rows[name]
                out[f"embedding_dict.{name}.weight"] = (self.m[lo:lo + cnt], self.v[lo:lo + cnt])
        if self.wm is not None:
            out["weight"] = (self.wm, self.wv)
        return out


class TableAdam(torch.optim.Optimizer):
    """See the module docstring.  `modules`: FeatureEmbedding / LinearModel instances (one optimizer per module).  `arith`: "fast"
    or "exact" (satrans_adam_hparams.arith) for the tables; `lazy`, `flush_every` as the engine's (on, 32; `flush_every=None`
    flushes only on request); `linear_lazy`: the lazy form for LinearModel's 1-wide tables too.
    `state_dict()` -> {"kind": "adam", "step": t, "state": {"<i>.<state_dict key of modules[i]>": {"exp_avg", "exp_avg_sq"}}} with
    CPU tensors, the layout of BaseModel.optimizer_state_dict with the module's position in front of its keys;
    `load_state_dict` takes it back (every row then stands at `step`)."""

    def __init__(self, modules, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, l2_reg_embedding=1e-5, l2_reg_linear=1e-5, arith="fast",
                 lazy=True, flush_every=32, linear_lazy=False, weight_decay=0, amsgrad=False, maximize=False,
                 track_regularizer=False):
        from .layers import FeatureEmbedding, LinearModel
        for name, val in (("weight_decay", weight_decay), ("amsgrad", amsgrad), ("maximize", maximize)):
            if val:
                raise NotImplementedError(f"TableAdam: {name} is not built (the regulariser is l2_reg_embedding / l2_reg_linear)")
        if arith not in ARITH:
            raise ValueError(f"TableAdam: arith {arith!r} is not one of {sorted(ARITH)}")
        if not lr >= 0.0 or not eps >= 0.0 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"TableAdam: lr {lr}, betas {betas}, eps {eps}")
        if flush_every is not None and int(flush_every) < 0:
            raise ValueError(f"TableAdam: flush_every {flush_every}")
        modules = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
        if not modules:
            raise ValueError("TableAdam: no module to adopt")
        for mod in modules:
            if not isinstance(mod, (FeatureEmbedding, LinearModel)):
                raise TypeError(f"TableAdam adopts FeatureEmbedding and LinearModel, not {type(mod).__name__}")
        for i, mod in enumerate(modules):
            if getattr(mod, "_table_opt", None) is not None or any(mod is other for other in modules[:i]):
                raise ValueError(f"TableAdam: this {type(mod).__name__} is already adopted by a TableAdam (one optimizer per module)")
        if track_regularizer and linear_lazy:
            raise NotImplementedError("TableAdam: track_regularizer with linear_lazy=True (the lazy 1-wide kernels write no partial "
                                      "sums of the regulariser, and a postponed row is not at its pre-step value)")
        self.arith, self.lazy, self.linear_lazy = arith, bool(lazy), bool(linear_lazy)
        self.track_regularizer = bool(track_regularizer)
        self._reg_sum = {}               # device -> [1] fp64
        self.flush_every = int(flush_every) if flush_every else 0
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.t = 0                       # completed steps
        self._since_flush = 0
        self._steps = StepTable(self.betas)
        self._adopted: List[_Adopted] = []
        params = [p for mod in modules for p in mod.parameters()]
        super().__init__(params, dict(lr=lr, betas=self.betas, eps=self.eps))
        for mod in modules:
            embedding = isinstance(mod, FeatureEmbedding)
            rec = _Adopted(self, mod, "embedding" if embedding else "linear", l2_reg_embedding if embedding else l2_reg_linear)
            self._adopted.append(rec)
            mod._table_opt = rec
            mod.register_state_dict_pre_hook(lambda _mod, _prefix, _keep, opt=self: opt.flush())

    def add_param_group(self, param_group):
        if self.param_groups:
            raise NotImplementedError("TableAdam: one param group, the adopted modules' parameters")
        return super().add_param_group(param_group)

    # ---- constants -------------------------------------------------------------------------------------------------------------
    def hparams(self, l2: float, arith: str) -> N.AdamHParams:
        """The constants of step `self.t` as the step kernels take them (the replay and flush kernels read lr / (1 - beta1^s) and
        sqrt(1 - beta2^s) from the per-step table instead)."""
        b1, b2 = self.betas
        t = max(self.t, 1)
        h = N.AdamHParams()
        h.lr_over_bc1 = float(self.param_groups[0]["lr"]) / (1.0 - b1 ** t)
        h.bc2_sqrt = math.sqrt(1.0 - b2 ** t)
        h.beta1, h.beta2, h.eps, h.l2 = b1, b2, self.eps, l2
        h.arith = ARITH[arith]
        return h

    def table(self, dev) -> torch.Tensor:
        return self._steps.device(self.t, dev)

    # ---- the regulariser's value ------------------------------------------------------------------------------------------------
    def _reg_total(self, dev) -> torch.Tensor:
        if dev not in self._reg_sum:
            self._reg_sum[dev] = torch.zeros(1, dtype=torch.float64, device=dev)
        return self._reg_sum[dev]

    def _add_reg(self, partials, count: int, dev) -> None:
        """total += the first `count` partial sums a step, replay or flush kernel has just written (one launch, index order)."""
        if self.track_regularizer:
            N.check(N.lib().satrans_sum_f64(partials.data_ptr(), int(count), self._reg_total(dev).data_ptr(), 1, N.stream_handle(dev)),
                    "satrans_sum_f64")

    def _add_reg_of(self, p, l2: float) -> None:
        """total += l2 * sum(p^2) of a buffer that steps by satrans_adam_flat, which writes no partial sums: a torch reduction over
        its pre-step values, in double."""
        if self.track_regularizer and l2 != 0.0:
            self._reg_total(p.device).add_(l2 * torch.sum(torch.square(p.detach().double())))

    def regularization_sum(self) -> torch.Tensor:
        """The running total of the regulariser's VALUE, l2 * sum(p^2) over the adopted tables (and LinearModel.weight) at the
        pre-step values of every step taken, as a 0-dim float64 tensor on the modules' device - what the reference adds to each
        step's loss (`get_regularization_loss` at loss time), summed over the steps.  Needs `track_regularizer=True`.  Never
        synchronises.  In the lazy form a row's postponed steps enter the total when they are replayed, so the total equals the
        streaming form's only after `flush()`.  `zero_regularization_sum()` starts a new total (an epoch's)."""
        if not self.track_regularizer:
            raise RuntimeError("TableAdam.regularization_sum: the optimizer was built with track_regularizer=False")
        parts = [self._reg_total(dev) for dev in dict.fromkeys(rec.dev for rec in self._adopted)]
        total = parts[0][0].clone()
        for part in parts[1:]:
            total = total + part[0].to(total.device)
        return total

    def zero_regularization_sum(self) -> None:
        for t in self._reg_sum.values():
            t.zero_()

    # ---- the step --------------------------------------------------------------------------------------------------------------
    def _drop_all(self) -> None:
        for rec in self._adopted:
            rec.drop()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("TableAdam.step: a closure is not supported")
        for rec in self._adopted:
            rec.check_device()
        missing = [type(rec.mod).__name__ for rec in self._adopted if rec.pending is None]
        if missing:
            self._drop_all()
            raise RuntimeError(f"TableAdam.step: no pending gradient for {', '.join(missing)}: every adopted module needs a forward "
                               f"and a backward before each step (pending gradients of the other modules are dropped)")
        stale = [type(rec.mod).__name__ for rec in self._adopted if rec.pending[4] != self.t]
        if stale:
            self._drop_all()
            raise RuntimeError(f"TableAdam.step: the forward of {', '.join(stale)} was made before an earlier step() (at another "
                               f"step count than {self.t}): its rows and gradient are out of date (the pending gradients are "
                               f"dropped; run forward and backward again)")
        self.t += 1
        self._steps.note(self.t, float(self.param_groups[0]["lr"]))
        for rec in self._adopted:
            rec.step(self.t)
        self._since_flush += 1
        if self.flush_every and self._since_flush >= self.flush_every:
            self.flush()
        return None

    @torch.no_grad()
    def flush(self) -> None:
        """Bring every row of every adopted table to step `t` (a no-op when no step is postponed)."""
        if self._since_flush == 0:
            return
        for rec in self._adopted:
            rec.check_device()
        for rec in self._adopted:
            rec.flush(self.t)
        self._since_flush = 0

    # ---- state -----------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        self.flush()
        state = {}
        for i, rec in enumerate(self._adopted):
            for key, (m, v) in rec.moments().items():
                state[f"{i}.{key}"] = {"exp_avg": m.detach().cpu().clone(), "exp_avg_sq": v.detach().cpu().clone()}
        return {"kind": "adam", "step": int(self.t), "state": state}

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        if state_dict.get("kind", "adam") != "adam":
            raise ValueError(f"TableAdam: optimizer state of kind {state_dict.get('kind')!r}")
        want = {f"{i}.{key}" for i, rec in enumerate(self._adopted) for key in rec.moments()}
        if set(state_dict["state"]) != want:
            raise ValueError(f"TableAdam.load_state_dict: keys {sorted(set(state_dict['state']) ^ want)} do not match the adopted modules")
        for rec in self._adopted:
            rec.check_device()
        self._drop_all()
        for i, rec in enumerate(self._adopted):
            for key, (m, v) in rec.moments().items():
                st = state_dict["state"][f"{i}.{key}"]
                m.copy_(st["exp_avg"].to(rec.dev))
                v.copy_(st["exp_avg_sq"].to(rec.dev))
        self.t = int(state_dict["step"])
        for rec in self._adopted:
            if rec.last is not None:
                rec.last.fill_(self.t)       # the state was taken after a flush: every row is current
        self._since_flush = 0
        self._steps = StepTable(self.betas, cap=max(4096, 2 * (self.t + 1)))      # (earlier steps are never replayed again)
