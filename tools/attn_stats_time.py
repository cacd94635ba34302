"""Cost of the scenario attention maps (predict's 'showattn' / attention_statistics, csrc/attn_stats.hip) at the prediction batch of
32,768 samples, for the AliCCP shape (configs[1]: 19 fields, 4 heads, 3 layers) and the configs[4] shape (64 fields, embedding_dim 64,
4 heads, 6 layers; tables scaled down, which the attention does not see):
  - predict() wall time per 32,768 samples with and without 'showattn' (host upload and read-back included);
  - the evaluation forward alone on resident data, per batch (CUDA events): plain, and with the statistics context (every layer
    writes its attention, the statistics call runs behind it);
  - one statistics call on one layer's attention [H, 32768, F, F] (CUDA events around the call: key shift, grouping, block sums,
    fold) and its effective read bandwidth H*B*F*F*4 bytes / time.  Per-kernel dispatch times: run under
    `rocprofv3 --kernel-trace --stats -- python tools/attn_stats_time.py`.
Usage: python tools/attn_stats_time.py [--batches 8] [--configs aliccp,c5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from satrans_amd import attn_stats as AS  # noqa: E402

B = 32768
HBM_READ_GBS = 6300.0          # streaming rate MI355X_MICROARCH.md measured (the read roof used below)


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


def run(name, n_batches):
    cfg = bench.make_config(name, 2_000_000) if name == "c5" else bench.make_config(name)
    n = n_batches * B
    X, _ = bench.synth_batches(n, 3, cfg=cfg)
    y = (np.random.RandomState(4).rand(n) < 0.3).astype(np.float64)
    dom = X[:, cfg["fields"].index(cfg["domain"])].astype(np.int64)
    model = bench.build_model("cuda:0", 0.005, cfg=cfg)
    eng = model._require_engine()
    S = cfg["n_domains"]
    res = dict(config=name, F=eng.F, H=eng.H, L=eng.L, D=eng.D, batch=B, samples=n)

    def predict_ms(show):
        model.flag = cfg["flag"] + ("-showattn" if show else "")
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.predict(X, B, y, dom)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / n_batches)
        return median(ts)

    predict_ms(False)                                   # warm-up (workspaces, buffers)
    predict_ms(True)
    res["predict_ms_per_32768"] = predict_ms(False)
    res["predict_showattn_ms_per_32768"] = predict_ms(True)
    model.flag = cfg["flag"]

    # evaluation forward alone on resident data
    Xd = torch.from_numpy(np.ascontiguousarray(X[:B], dtype=np.float32)).cuda()
    keys = torch.from_numpy(AS.class_keys(dom[:B], y[:B], S, AS.scenario_bias(dom))).cuda()
    ctx = AS.AttentionStatistics(eng, S)
    ctx.set_batch(keys)
    model.eval()
    with torch.no_grad():
        res["forward_ms"] = events_ms(lambda: eng.forward(Xd, training=False), 20)
        res["forward_stats_ms"] = events_ms(lambda: eng.forward(Xd, training=False, stats=ctx), 20)
        att = ctx.buffer(B)                             # the last layer's attention of the last forward
        res["stats_call_us"] = 1e3 * events_ms(lambda: ctx.accumulate(0, att, B, torch.cuda.current_stream().cuda_stream), 50)
    read = att.numel() * 4
    res["stats_read_MB"] = read / 1e6
    res["stats_call_GBs"] = read / (res["stats_call_us"] * 1e-6) / 1e9
    res["stats_call_fraction_of_read_roof"] = res["stats_call_GBs"] / HBM_READ_GBS
    res["attention_write_read_GB_per_batch"] = 2 * read * eng.L / 1e9
    print(json.dumps(res), flush=True)
    del model, eng, ctx, att
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--configs", default="aliccp,c5")
    a = ap.parse_args()
    for name in a.configs.split(","):
        run(name, a.batches if name != "c5" else max(2, a.batches // 4))


if __name__ == "__main__":
    main()
