"""sha256 of everything the scenario heads (csrc/mmoe.hip, ple.hip, sharedbottom.hip, adasparse.hip) compute, on the seeded
inputs of their GPU tests: per head its shape sweep, the walker-edges batch with task counts [0, DW_ROW_CHUNK, 0, ROW_TILE + 1]
and a batch of 5 rows; PLE at one and two levels, SharedBottom with and without a tower, SharedBottom and AdaSparse in both
forward modes (set_forward(0) fused, set_forward(1) composed).  AdaSparse routes nothing, so its walker-edges batch is a batch
of that many rows.  Per case one line per tensor: the logits, the whole saved buffer and every row of it that the module
exposes, dx (and demb) and every parameter gradient.  Only the public module API and the helpers of tests/*_reference.py are
used, so the same file runs in a checkout of another commit: two commits compute the same bits when the two outputs are equal.
Usage: python tools/heads_digest.py [--out FILE]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def counted_ids(counts):
    import torch
    ids = torch.cat([torch.full((n,), s, dtype=torch.long) for s, n in enumerate(counts)])
    return ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(41))]


def routed_cases(R, tile, chunk, edges, small):
    """(name, ids, offset, x, w, P) of a routed head: R.SWEEP, then the draws `edges(ids)` and `small(ids)`, lists of
    (label, (x, w, P))."""
    import torch
    for case in R.SWEEP:
        ids, x, w, P = R.sweep_draw(case, tile, chunk)
        yield f"sweep {case}", ids, R.SWEEP_OFFSET, x, w, P
    counts = [0, chunk, 0, tile + 1]
    ids = counted_ids(counts)
    for label, drawn in edges(ids):
        yield f"walker edges counts={counts}{label}", ids, 2, *drawn
    ids = torch.tensor([1, 1, 0, 1, 1])
    for label, drawn in small(ids):
        yield f"B=5{label}", ids, 0, *drawn


def mmoe():
    from satrans_amd import MMoEHead, native
    from tests import mmoe_reference as R
    for name, ids, off, x, w, P in routed_cases(
            R, native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK,
            lambda ids: [("", R.draw(ids.numel(), 33, 4, 3, (48, 32), (8,), (64,), 42, sid=ids))],
            lambda ids: [("", R.draw(5, 20, 3, 2, (24, 8), (8,), (), 5, sid=ids))]):
        units = lambda k: tuple(t.shape[1] for t in P[k])      # noqa: E731
        mod = MMoEHead(x.shape[1], P["out_bias"].shape[0], P["expert_w"][0].shape[0], units("expert_w"), units("gate_w"), units("tower_w"))
        mod.load_state_dict(R.state_from_params(P))
        yield name, mod, (x,), (ids, off), w, lambda m: [("last_gates", m.last_gates), ("last_mixture", m.last_mixture)]


def ple():
    from satrans_amd import PLEHead, native
    from tests import ple_reference as R
    for name, ids, off, x, w, P in routed_cases(
            R, native.PLE_ROW_TILE, native.PLE_DW_ROW_CHUNK,
            lambda ids: [(f" levels={lv}", R.draw(ids.numel(), 33, 4, 2, 1, lv, (48, 32), (8,), (64,), 42, sid=ids)) for lv in (1, 2)],
            lambda ids: [(f" levels={lv}", R.draw(5, 20, 3, 2, 1, lv, (24, 8), (8,), (), 5, sid=ids)) for lv in (1, 2)]):
        T, ns, nsh, two = R.sizes(P)
        units = lambda k: tuple(t.shape[-2] for t in P[k])      # noqa: E731
        mod = PLEHead(x.shape[1], T, nsh, ns, 2 if two else 1, units("spec_w"), units("gate_w"), units("tower_w"))
        mod.load_state_dict(R.state_from_params(P), strict=False)      # the parameters that take no part keep their seeded start
        yield name, mod, (x,), (ids, off), w, lambda m: [("last_gates", m.last_gates), ("last_mixture", m.last_mixture)]


def sharedbottom():
    from satrans_amd import SharedBottomHead, native
    from tests import sharedbottom_reference as R
    for name, ids, off, x, w, P in routed_cases(
            R, native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK,
            lambda ids: [(f" tower={t}", R.draw(ids.numel(), 33, 4, (48, 32), t, 42, sid=ids)) for t in ((24, 65), ())],
            lambda ids: [(f" tower={t}", R.draw(5, 20, 3, (24, 8), t, 5, sid=ids)) for t in ((8,), ())]):
        mod = SharedBottomHead(x.shape[1], P["out_bias"].shape[0], tuple(t.shape[0] for t in P["bottom_w"]),
                               tuple(t.shape[1] for t in P["tower_w"]))
        mod.load_state_dict(R.state_from_params(P))
        yield name, mod, (x,), (ids, off), w, lambda m: [("last_bottom", m.last_bottom)]


def adasparse():
    from satrans_amd import AdaSparseHead, native
    from tests import adasparse_reference as R
    tile, chunk = native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK
    drawn = [(f"sweep {case}", R.sweep_draw(case, chunk + tile + 1)) for case in R.SWEEP]
    drawn.append((f"B={chunk + tile + 1}, the rows of the walker-edges batch", R.draw(chunk + tile + 1, 33, 4, (48, 32), 42)))
    drawn.append(("B=5", R.draw(5, 20, 6, (24, 8), 5)))
    for name, (x, e, w, P) in drawn:
        mod = AdaSparseHead(x.shape[1], tuple(t.shape[0] for t in P["lin_w"]), domain_emb_dim=e.shape[1])
        mod.load_state_dict(R.state_from_params(P))
        mod.dnn.alpha, mod.dnn.beta, mod.dnn.epsilon = R.DEFAULTS
        yield name, mod, (x, e), (), w, lambda m: [(f"last_pi[{l}]", p) for l, p in enumerate(m.last_pi)]


def run(head, name, mod, inputs, extra, w, exposed):
    """The lines of one case: forward, backward of sum(logit * w), a digest per tensor."""
    mod = mod.to(DEV)
    mod.zero_grad(set_to_none=True)
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    ids = [extra[0].add(extra[1]).to(DEV), extra[1]] if extra else []
    y = mod(*leaves, *ids)
    (y * w.to(DEV)).sum().backward()
    rows = exposed(mod)
    out = [("logit", y), ("saved", rows[0][1]._base)] + rows + [(k, t.grad) for k, t in zip(("dx", "demb"), leaves)]
    out += [("g " + k, p.grad) for k, p in mod.named_parameters() if p.grad is not None]
    return [f"== {head}: {name}, B={inputs[0].shape[0]}"] + [f"{k:44s} {tuple(t.shape)!s:16s} {digest(t)}" for k, t in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from satrans_amd import native
    lib = native.lib()
    lines = []
    for head, cases, switch in (("mmoe", mmoe, None), ("ple", ple, None), ("sharedbottom", sharedbottom, lib.satrans_sharedbottom_set_forward),
                                ("adasparse", adasparse, lib.satrans_adasparse_set_forward)):
        torch.manual_seed(0)      # the start of the parameters that a case does not set
        for name, mod, inputs, extra, w, exposed in cases():
            if switch is None:
                lines += run(head, name, mod, inputs, extra, w, exposed)
                continue
            was = switch(0)
            try:
                for mode in (0, 1):
                    switch(mode)
                    lines += run(head, f"{name}, set_forward({mode})", mod, inputs, extra, w, exposed)
            finally:
                switch(was)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
