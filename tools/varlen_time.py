"""Cost of VarLenSparseFeat fields (csrc/pool.hip) at B = 8192: AliCCP (configs[1]: 19 fields) against AliCCP plus the reference's
four history columns (`main.py:102`, `:185-188`: VarLenSparseFeat(..., maxlen=3, combiner='max') over vocabularies of 12,523 /
2,981,271 / 99,555 / 426,101 rows, `main.py:124-128`), both on the runtime-F layer kernels where F is not 19.
Writes profiles/varlen_time.txt:
  - the pooled gather and the pooling backward alone (CUDA events around one launch, median), bytes moved and the fraction of
    the HBM peak that is;
  - ms/step of the training step (fit-style: next batch announced), total and by phase;
  - fp32 and bf16 predict() per 32,768 samples (wall time, host upload and read-back included).
Usage: python tools/varlen_time.py [--steps 20] [--out profiles/varlen_time.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

B = 8192
HBM_PEAK_GBS = 8000.0                  # MI355X HBM3E peak (MI355X_MICROARCH.md)
HIST = {"10914": 12523, "11014": 2981271, "15014": 99555, "12714": 426101}
MAXLEN = 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def events_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return median(out)


def build(history: bool):
    from satrans_amd import SATrans, SparseFeat, VarLenSparseFeat
    cfg = bench.make_config("aliccp")
    cols = [SparseFeat(f, vocabulary_size=cfg["maxima"][f] + 2, embedding_dim=cfg["D"]) for f in cfg["fields"]]
    if history:
        cols += [VarLenSparseFeat(SparseFeat(c, v, embedding_dim=cfg["D"]), maxlen=MAXLEN, combiner="max") for c, v in HIST.items()]
    model = SATrans(cols, cols, [cfg["domain"]], [cfg["n_domains"]], att_layer_num=0, domain_att_layer_num=cfg["L"],
                    att_head_num=cfg["H"], use_linear=False, use_dnn=False, meta_mode='QK', meta_dnn_hidden_units=cfg["units"],
                    seed='1021', device="cuda:0", flag=cfg["flag"])
    model.compile(torch.optim.Adam(model.parameters(), lr=cfg["lr"]), "binary_crossentropy")
    return model, cfg


def data(n, seed, history, cfg):
    X, y = bench.synth_batches(n, seed, cfg=cfg)
    if not history:
        return X, y
    rng = np.random.RandomState(seed + 1)
    blocks = []
    for v in HIST.values():           # top-k lists padded with 0 (aliccp_dataset_processing.py: generate_topk_history_features)
        ids = rng.randint(1, v, size=(n, MAXLEN))
        keep = np.arange(MAXLEN)[None, :] < rng.randint(0, MAXLEN + 1, size=(n, 1))
        blocks.append(np.where(keep, ids, 0))
    return np.concatenate([X] + [b.astype(np.float32) for b in blocks], axis=1), y


def run(history, steps, lines):
    model, cfg = build(history)
    eng = model._require_engine()
    X, y = data(B * (steps + 6), 7, history, cfg)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    name = "AliCCP + 4 histories (maxlen 3, max)" if history else "AliCCP"
    lines.append(f"== {name}: F = {eng.F}, row slots R = {eng.R}, arena rows = {eng.total_rows:,}, layer path "
                 f"{'fused' if not eng.workspace(B)['generic'] else 'generic'}")
    model.train()
    batches = [(Xd[i * B:(i + 1) * B], yd[i * B:(i + 1) * B]) for i in range(steps + 6)]
    for i in range(5):
        eng.train_step(*batches[i], next_X=batches[i + 1][0])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(5, 5 + steps):
        eng.train_step(*batches[i], next_X=batches[i + 1][0])
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / steps
    lines.append(f"training step: {ms:.3f} ms/step ({B / ms / 1e3:.2f} M samples/s), {steps} steps")
    eng.flush_lazy()
    eng.timers = {}
    for i in range(5, 5 + min(steps, 10)):
        eng.train_step(*batches[i])
    torch.cuda.synchronize()
    phases = eng.phase_ms()
    eng.timers = None
    lines.append("  by phase (events, unpipelined steps, median ms): " +
                 ", ".join(f"{k} {v:.3f}" for k, v in sorted(phases.items(), key=lambda kv: -kv[1])))
    if history:
        ws = eng.train_workspace(B, 1, False)
        Xb = batches[0][0]
        g_ms = events_ms(lambda: eng._pool_gather(Xb, ws, ws["acts"][0]), 30)
        D, F, R = eng.D, eng.F, eng.R
        rd = B * R * D * 4 + B * Xb.shape[1] * 4
        wr = B * F * D * 4 + B * R * 4 + B * eng.Fv * (4 + D)
        lines.append(f"pooled gather: {g_ms * 1e3:.1f} us, {rd / 1e6:.1f} MB read + {wr / 1e6:.1f} MB written = "
                     f"{(rd + wr) / g_ms / 1e6:.0f} GB/s = {(rd + wr) / g_ms / 1e6 / HBM_PEAK_GBS:.2f} of the {HBM_PEAK_GBS:.0f} GB/s "
                     f"HBM peak (rows: {rd / g_ms / 1e6 / HBM_PEAK_GBS:.2f} in reads alone)")
        dx = torch.randn(B, F, D, device="cuda:0")
        b_ms = events_ms(lambda: eng._pool_backward(dx, ws, B), 30)
        rd, wr = B * F * D * 4 + B * eng.Fv * (4 + D), B * R * D * 4
        lines.append(f"pooling backward: {b_ms * 1e3:.1f} us, {rd / 1e6:.1f} MB read + {wr / 1e6:.1f} MB written = "
                     f"{(rd + wr) / b_ms / 1e6:.0f} GB/s = {(rd + wr) / b_ms / 1e6 / HBM_PEAK_GBS:.2f} of peak")
    model.eval()
    Xp, _ = data(32768, 9, history, cfg)
    for prec in ("fp32", "bf16"):
        model.set_forward_precision(prec)
        model.predict(Xp, batch_size=32768)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            model.predict(Xp, batch_size=32768)
            ts.append(time.perf_counter() - t0)
        lines.append(f"predict {prec}: {median(ts) * 1e3:.3f} ms per 32,768 samples (wall, upload and read-back included)")
    model.set_forward_precision("fp32")
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_time.txt"))
    a = ap.parse_args()
    lines = [f"tools/varlen_time.py on {torch.cuda.get_device_name(0)}, B = {B}"]
    base = run(False, a.steps, lines)
    var = run(True, a.steps, lines)
    lines.append(f"step ratio, with histories / without: {var / base:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
