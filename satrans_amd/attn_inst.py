"""Instance-level attention: the maps of chosen test samples and the search for samples whose attention shows a pattern
(predict's `inst_attn_dict` and 'instattn' branches, reference models/meta_basemodel.py:440-445, 460-499).

A pattern is an `AttentionRule`: in some head of one layer, field q attends to field k above a threshold; such atoms combine with
"and" / "or" (a conjunction of clauses, each a disjunction of atoms) and with filters on the label and on input columns.  The
(sample, head) pairs that satisfy a rule are found on the device (csrc/attn_inst.hip) right behind the layer's forward, in the
attention buffer of the batch; only the matches' maps, probabilities and input rows reach the host.

Deliberate deviations from the reference: the matches are listed by sample index, then head, then rule - the reference walks
head-major inside every batch, so its file order changes with batch_size; the rules are data (`model.instattn_rules`), where the
reference hard-codes two of them for Alimama's columns together with a `classes_` attribute nothing sets.
"""
from __future__ import annotations

import operator
from typing import Optional, Sequence

import numpy as np
import torch

from . import native as N

ATTN_MATCH_DTYPE = np.dtype([("index", "<i8"), ("head", "<i4"), ("rule", "<i4")])      # satrans_attn_match
_OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}


class AttentionRule:
    """clauses: a conjunction of clauses; a clause is one atom `(query_field, key_field, threshold)` or a list of up to 4 of them
    (a disjunction); at most 8 clauses.  Fields are indices into the layer's field order or feature names (the SparseFeat fields,
    then the pooled VarLenSparseFeat ones).  `label`: only samples with y == label; `where`: column predicates
    `(feature, op, value)`, op one of == != < <= > >=, all of which must hold on the sample's input row.

    The reference's second rule, att[15][7] > t and (att[15][5] > t or att[15][8] > t), reads
    AttentionRule([(15, 7, t), [(15, 5, t), (15, 8, t)]])."""

    def __init__(self, clauses, label=None, where: Sequence = ()):
        def is_atom(c):
            return isinstance(c, tuple) and len(c) == 3 and not isinstance(c[0], (tuple, list))
        if is_atom(clauses):
            clauses = [clauses]
        self.clauses = [[tuple(c)] if is_atom(c) else [tuple(a) for a in c] for c in clauses]
        self.label = label
        self.where = [tuple(w) for w in where]
        if not 1 <= len(self.clauses) <= N.ATTN_MAX_CLAUSES:
            raise ValueError(f"a rule has 1..{N.ATTN_MAX_CLAUSES} clauses, got {len(self.clauses)}")
        for c in self.clauses:
            if not 1 <= len(c) <= N.ATTN_MAX_ATOMS:
                raise ValueError(f"a clause has 1..{N.ATTN_MAX_ATOMS} atoms, got {len(c)}")
            for a in c:
                if len(a) != 3:
                    raise ValueError(f"an atom is (query_field, key_field, threshold), got {a!r}")
                if not np.isfinite(float(a[2])):
                    raise ValueError(f"threshold {a[2]!r} is not finite")
        for w in self.where:
            if len(w) != 3 or w[1] not in _OPS:
                raise ValueError(f"a column predicate is (feature, op, value) with op in {sorted(_OPS)}, got {w!r}")

    def resolve(self, field_names: Sequence[str]) -> N.AttnRule:
        """The C struct, with feature names resolved against the layer's field order."""
        names = list(field_names)
        F = len(names)

        def field(f):
            if isinstance(f, str):
                if f not in names:
                    raise ValueError(f"'{f}' is not a field of the attention layers; the fields are {names}")
                return names.index(f)
            if isinstance(f, (bool, np.bool_)) or not isinstance(f, (int, np.integer)):
                raise ValueError(f"a field is an index or a feature name, got {f!r}")
            if not 0 <= int(f) < F:
                raise ValueError(f"field {int(f)} outside [0, {F})")
            return int(f)

        r = N.AttnRule()
        r.n_clauses = len(self.clauses)
        for ci, c in enumerate(self.clauses):
            r.n_atoms[ci] = len(c)
            for ai, (q, k, thr) in enumerate(c):
                r.atoms[ci][ai].q, r.atoms[ci][ai].k, r.atoms[ci][ai].thr = field(q), field(k), float(thr)
        return r


def layer_field_names(model) -> list:
    """The field order of the attention maps: the SparseFeat fields, then the pooled VarLenSparseFeat ones."""
    from .inputs import split_columns
    sparse, _, varlen = split_columns(model.dnn_feature_columns)
    return [c.name for c in sparse] + [c.name for c in varlen]


def resolve_rules(rules, field_names) -> "C array of AttnRule":
    """AttentionRule list -> (satrans_attn_rule * n), validated by the library (no device needed)."""
    rules = list(rules)
    if not 1 <= len(rules) <= N.ATTN_MAX_RULES:
        raise ValueError(f"1..{N.ATTN_MAX_RULES} rules per pass, got {len(rules)}")
    for r in rules:
        if not isinstance(r, AttentionRule):
            raise ValueError(f"rules are AttentionRule objects, got {type(r).__name__}")
    arr = (N.AttnRule * len(rules))(*[r.resolve(field_names) for r in rules])
    N.check(N.lib().satrans_attn_inst_check_rules(arr, len(rules), len(list(field_names))), "satrans_attn_inst_check_rules")
    return arr


def eligibility(rules, x, y, feature_index) -> "uint8 [B]":
    """Bit r set where sample b passes rule r's label and column filters.  x: [B, C] (a torch tensor: torch ops, on its device;
    numpy otherwise), y: [B] or None, feature_index: feature name -> (first column, end)."""
    xp = torch if isinstance(x, torch.Tensor) else np
    B = x.shape[0]
    bits = torch.zeros(B, dtype=torch.uint8, device=x.device) if xp is torch else np.zeros(B, dtype=np.uint8)
    for r, rule in enumerate(rules):
        ok = torch.ones(B, dtype=torch.bool, device=x.device) if xp is torch else np.ones(B, dtype=bool)
        if rule.label is not None:
            if y is None:
                raise ValueError("a rule with a label filter needs the labels: pass y")
            ok = ok & (y.reshape(-1) == rule.label)
        for feature, op, value in rule.where:
            if feature not in feature_index:
                raise ValueError(f"'{feature}' is not a feature of the model; the features are {list(feature_index)}")
            ok = ok & _OPS[op](x[:, feature_index[feature][0]], value)
        bits = bits | (ok.to(torch.uint8) << r if xp is torch else (ok.astype(np.uint8) << np.uint8(r)))
    return bits


class AttentionInstances:
    """Device side of one pass: the match list (records, maps, probabilities, input rows; `capacity` entries), its device total,
    the match kernel's workspace and what the next forward needs (`set_batch`).  PathEngine.forward(..., inst=ctx) writes the
    wanted layer's attention into a buffer - the statistics context's when both are active - and queues the search and the copy
    of the matches' maps and rows behind that layer, the copy of their probabilities behind the head.

    rules: a resolved rule array (`resolve_rules`) for the search; or None and `records` (`hand_records`): nothing is searched,
    every batch copies out the listed records that name one of its samples (the capacity is the list's length)."""

    def __init__(self, engine, rules, layer: int, capacity: int = 0, records: Optional[np.ndarray] = None):
        eng = self.eng = engine
        if not 0 <= int(layer) < eng.L:
            raise ValueError(f"layer {layer} outside [0, {eng.L})")
        if not 1 <= eng.H <= N.ATTN_MAX_HEADS:
            raise NotImplementedError(f"instance-level attention with {eng.H} heads (1..{N.ATTN_MAX_HEADS})")
        if (rules is None) == (records is None):
            raise ValueError("attention instances: either rules or a hand-built record list")
        if records is not None:
            capacity = records.shape[0]
        if capacity < 0:
            raise ValueError(f"capacity {capacity}")
        self.rules, self.n_rules = rules, (len(rules) if rules is not None else 0)
        self.layer, self.capacity = int(layer), int(capacity)
        self.records = torch.zeros(max(self.capacity, 1), 2, dtype=torch.int64, device=eng.dev)     # 16 bytes per record
        if records is not None and self.capacity:
            self.records.copy_(torch.from_numpy(np.ascontiguousarray(records, dtype=np.int64)))
        self.maps = torch.zeros(max(self.capacity, 1), eng.F, eng.F, dtype=torch.float32, device=eng.dev)
        self.pred = torch.zeros(max(self.capacity, 1), dtype=torch.float32, device=eng.dev)
        self.total = torch.zeros(1, dtype=torch.int64, device=eng.dev)
        self._range = torch.zeros(2, dtype=torch.int64, device=eng.dev)
        self.x_rows = None                       # allocated at the first batch: the engine's matrix decides dtype and width
        self._att = self._ws = self._eligible = None
        self._span = (0, 0, None)
        self._first = 0

    def wants(self, l: int) -> bool:
        return l == self.layer

    def set_batch(self, first_index: int, eligible: Optional[torch.Tensor] = None) -> None:
        """Before every forward.  first_index: global index of the batch's sample 0.  eligible: uint8 [B] rule bits on the device
        (None: every rule may match every sample; unused with a hand-built list)."""
        if eligible is not None and (eligible.dtype != torch.uint8 or not eligible.is_cuda or not eligible.is_contiguous()):
            raise ValueError("eligible must be a contiguous uint8 device tensor")
        self._first, self._eligible = int(first_index), eligible

    def buffer(self, B: int) -> torch.Tensor:
        eng = self.eng
        need = eng.H * B * eng.F * eng.F
        if self._att is None or self._att.numel() < need:
            self._att = torch.empty(need, dtype=torch.float32, device=eng.dev)
        return self._att[:need].view(eng.H, B, eng.F, eng.F)

    def _x_view(self, X: torch.Tensor):
        """(pointer, row stride in dwords, dwords per row) of the engine's input matrix; allocates x_rows to match."""
        w = X.element_size() // 4
        if self.x_rows is None:
            self.x_rows = torch.zeros(max(self.capacity, 1), X.shape[1], dtype=X.dtype, device=X.device)
        elif self.x_rows.dtype != X.dtype or self.x_rows.shape[1] != X.shape[1]:
            raise ValueError("the input matrix changed its dtype or width within one pass")
        return X.data_ptr(), X.stride(0) * w, X.shape[1] * w

    def search(self, l: int, att: torch.Tensor, X: torch.Tensor, B: int, stream) -> None:
        """Behind layer l's forward: find this batch's matches (or take the hand-built range) and copy their maps and rows."""
        eng, lib = self.eng, self.eng.lib
        if self.rules is not None:
            if self._eligible is not None and self._eligible.shape[0] != B:
                raise ValueError(f"attention instances: eligibility of {B} samples expected")
            need = int(lib.satrans_attn_inst_workspace_bytes(B, eng.H, eng.F))
            N.check(0 if need >= 0 else need, "satrans_attn_inst_workspace_bytes")
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=eng.dev)
            N.check(lib.satrans_attn_inst_match(att.data_ptr(), B, eng.H, eng.F, self.rules, self.n_rules, N.ptr(self._eligible),
                                                self._first, self.records.data_ptr(), self.capacity, self.total.data_ptr(),
                                                self._range.data_ptr(), self._ws.data_ptr(), self._ws.numel(), stream),
                    "satrans_attn_inst_match")
            self._span = (0, self.capacity, self._range.data_ptr())
        else:
            self._span = (0, self.capacity, None)
        if self.capacity == 0:
            return
        xp, xs, xw = self._x_view(X)
        m0, m1, rng = self._span
        N.check(lib.satrans_attn_inst_gather(att.data_ptr(), B, eng.H, eng.F, self.records.data_ptr(), m0, m1, rng, self._first,
                                             self.maps.data_ptr(), None, None, xp, xs, xw, self.x_rows.data_ptr(), stream),
                "satrans_attn_inst_gather")

    def finish_batch(self, prob: torch.Tensor, B: int, stream) -> None:
        """Behind the head: the probabilities of this batch's records."""
        if self.capacity == 0:
            return
        eng, lib = self.eng, self.eng.lib
        m0, m1, rng = self._span
        N.check(lib.satrans_attn_inst_gather(None, B, eng.H, eng.F, self.records.data_ptr(), m0, m1, rng, self._first, None,
                                             prob.data_ptr(), self.pred.data_ptr(), None, 0, 0, None, stream),
                "satrans_attn_inst_gather")

    def result(self, y=None) -> dict:
        """The list on the host (synchronises)."""
        total = int(self.total.item()) if self.rules is not None else self.capacity
        M = min(total, self.capacity)
        rec = self.records[:M].cpu().numpy().view(ATTN_MATCH_DTYPE).reshape(M)
        out = {"index": np.ascontiguousarray(rec["index"]), "head": np.ascontiguousarray(rec["head"]),
               "rule": np.ascontiguousarray(rec["rule"]), "pred": self.pred[:M].cpu().numpy().astype(np.float64)}
        if y is not None:
            out["label"] = np.asarray(y).reshape(-1)[out["index"]]
        out["attention"] = self.maps[:M].cpu().numpy()
        out["x"] = self.x_rows[:M].cpu().numpy() if self.x_rows is not None else np.zeros((0, 0), dtype=np.float32)
        out["total"], out["truncated"] = total, total > self.capacity
        return out


def hand_records(sample_ids, H: int) -> np.ndarray:
    """int64 [n H, 2] satrans_attn_match rows: every head of every listed sample in the given order, rule -1."""
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    rec = np.zeros(ids.shape[0] * H, dtype=ATTN_MATCH_DTYPE)
    rec["index"] = np.repeat(ids, H)
    rec["head"] = np.tile(np.arange(H, dtype=np.int32), ids.shape[0])
    rec["rule"] = -1
    return rec.view(np.int64).reshape(-1, 2)


def _num(v) -> str:
    return str(v.item() if hasattr(v, "item") else v)


def write_instances(path: str, result: dict) -> None:
    """Three lines per match, the reference's layout (meta_basemodel.py:475-480) with the rule, head and sample index where it
    prints its two Alimama columns: `score {pred},label {label},rule {r},head {h},index {i}`, the map's F*F values joined by
    commas with a trailing comma, and the input row in the same style.  Numbers print as Python prints them (repr: they read
    back exactly); the label is `nan` when no labels were given."""
    label = result.get("label")
    with open(path, "w") as f:
        for m in range(len(result["index"])):
            lab = _num(label[m]) if label is not None else "nan"
            f.write(f"score {_num(result['pred'][m])},label {lab},rule {int(result['rule'][m])},head {int(result['head'][m])},"
                    f"index {int(result['index'][m])}\n")
            f.write(",".join(str(v) for v in result["attention"][m].reshape(-1).tolist()) + ",\n")
            f.write(",".join(str(v) for v in result["x"][m].tolist()) + ",\n")


def read_instances(path: str) -> dict:
    """The inverse of write_instances (maps come back flat, [M, F*F]; F is its square root)."""
    out = {k: [] for k in ("pred", "label", "rule", "head", "index", "attention", "x")}
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) % 3:
        raise ValueError(f"{path}: {len(lines)} lines, not three per match")
    for i in range(0, len(lines), 3):
        head = dict(part.split(" ", 1) for part in lines[i].split(","))
        out["pred"].append(float(head["score"]))
        out["label"].append(float(head["label"]))
        for k in ("rule", "head", "index"):
            out[k].append(int(head[k]))
        for k, line in (("attention", lines[i + 1]), ("x", lines[i + 2])):
            if not line.endswith(","):
                raise ValueError(f"{path}: line {i + 2} lacks the trailing comma")
            out[k].append([float(v) for v in line[:-1].split(",")])
    M = len(out["index"])
    return {"pred": np.asarray(out["pred"], dtype=np.float64), "label": np.asarray(out["label"], dtype=np.float64),
            "rule": np.asarray(out["rule"], dtype=np.int32), "head": np.asarray(out["head"], dtype=np.int32),
            "index": np.asarray(out["index"], dtype=np.int64),
            "attention": np.asarray(out["attention"], dtype=np.float32).reshape(M, -1 if M else 0),
            "x": np.asarray(out["x"], dtype=np.float64).reshape(M, -1 if M else 0)}
