"""sha256 of everything STAR's towers (csrc/star.hip) compute, on the seeded inputs of tests/test_star_gpu.py: the four shapes of
the shape sweep, the walker-edges case and the batch smaller than a tile.  Per case one line per tensor: the logits, every
saved hidden row, dx and every parameter gradient.  Only the public module API is used, so the same file runs in a checkout of
another commit: two commits compute the same bits when the two outputs are equal.
Usage: python tools/star_digest.py [--out FILE]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
OFFSET = 2


def cases():
    import torch
    from satrans_amd import native
    from tests import star_reference as R
    tile, chunk = native.STAR_ROW_TILE, native.STAR_DW_ROW_CHUNK
    for C, hidden in ((1, (16,)), (33, (48, 32)), (609, (256, 128)), (64, (16, 16, 16, 16))):
        ids = R.sweep_ids(tile, chunk)
        yield f"sweep C={C} hidden={hidden}", C, hidden, 5, ids, 1000 + C, OFFSET
    counts = [0, chunk, 0, tile + 1]
    ids = torch.cat([torch.full((n,), s) for s, n in enumerate(counts)])
    ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(41))]
    yield f"walker edges counts={counts}", 33, (48, 32), 4, ids, 42, OFFSET
    yield "B=5 < tile", 20, (24, 8), 3, torch.full((5,), 1), 5, 0


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from satrans_amd import StarTowers
    from tests import star_reference as R
    lines = []
    for name, C, hidden, S, ids, seed, offset in cases():
        x, w, P = R.draw(ids.numel(), C, hidden, S, seed)
        mod = StarTowers(C, hidden, S)
        H = len(hidden)
        dom = [[mod.domain_dnns[s].linears[l] for s in range(S)] for l in range(H)] + [list(mod.domain_dnn_linears)]
        sh = list(mod.shared_dnn.linears) + [mod.shared_dnn_linear]
        with torch.no_grad():
            for l in range(H + 1):
                for s in range(S):
                    dom[l][s].weight.copy_(P["w_dom"][l][s])
                    dom[l][s].bias.copy_(P["b_dom"][l][s])
                sh[l].weight.copy_(P["w_sh"][l])
                sh[l].bias.copy_(P["b_sh"][l])
        mod = mod.to(DEV)
        xg = x.to(DEV).requires_grad_(True)
        y = mod(xg, (ids + offset).to(DEV), offset)
        (y * w.to(DEV)).sum().backward()
        out = [("logit", y)] + [(f"hidden[{l}]", h) for l, h in enumerate(mod.last_hidden)] + [("dx", xg.grad)]
        for l in range(H + 1):
            out.append((f"g_w_dom[{l}]", torch.stack([m.weight.grad for m in dom[l]])))
            out.append((f"g_b_dom[{l}]", torch.stack([m.bias.grad for m in dom[l]])))
            out += [(f"g_w_sh[{l}]", sh[l].weight.grad), (f"g_b_sh[{l}]", sh[l].bias.grad)]
        lines.append(f"== {name}, S={S}, B={ids.numel()}, id offset {offset}")
        lines += [f"{k:12s} {tuple(t.shape)!s:18s} {digest(t)}" for k, t in out]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
