#!/usr/bin/env python
"""The non-SATrans branches of the reference's main.py (main.py:211-281, 338-374), all of them - WDL, DCN, DeepFM, xDeepFM, NFM,
AutoInt, AFM, FiBiNET, PNN, AdaSparse; SharedBottom, MMOE, PLE, ESMM; Star_Net - on the AliCCP columns, reading the h5 file with
h5lite as examples/aliccp_main.py does:

    python examples/aliccp_siblings.py --h5 /data/alicpp.h5 --model_name DeepFM --domain_col 301 --embedding_dim 32

MODEL(...), compile(torch.optim.Adam(model.parameters(), lr), "binary_crossentropy" (the multi-task models: one per task),
metrics), fit, then the test report of main.py:353-374 through `evaluate_domains`.  The flag is '' (main.py's metatrans / usetrans
switches are not built for these models).  xDeepFM trains on batches of 4096 (main.py:220-221).  AdaSparse takes domain_emb_dim =
--embedding_dim: its domain embedding is the scenario column's own.  ESMM is built as its class allows - main.py:262-265 hands it
`flag` and one task per scenario, which esmm.py:38-49 refuses - with two tasks and no flag: rows of the first two scenario ids
train and predict, the others take part in no loss and predict 0, as mtl_basemodel.py leaves them.  One process, one GPU."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.aliccp_main import DATA_MAX, SPARSE  # noqa: E402
from satrans_amd import (AFM, DCN, ESMM, MMOE, NFM, PLE, PNN, WDL, AdaSparse, AutoInt, DeepFM, FiBiNET, SharedBottom,  # noqa: E402
                         SparseFeat, Star_Net, get_feature_names, xDeepFM)
from satrans_amd.pipeline import load_h5_columns  # noqa: E402

MODELS = {"WDL": WDL, "DeepFM": DeepFM, "DCN": DCN, "xDeepFM": xDeepFM, "NFM": NFM, "AutoInt": AutoInt, "AFM": AFM, "FiBiNET": FiBiNET,
          "PNN": PNN, "AdaSparse": AdaSparse, "SharedBottom": SharedBottom, "MMOE": MMOE, "PLE": PLE, "ESMM": ESMM, "Star_Net": Star_Net}
MULTI_TASK = ("SharedBottom", "MMOE", "PLE", "ESMM")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--h5", required=True)
    ap.add_argument("--postfix", default="")
    ap.add_argument("--model_name", default="WDL", choices=sorted(MODELS))
    ap.add_argument("--domain_col", default="301")
    ap.add_argument("--embedding_dim", type=int, default=32)
    ap.add_argument("--learning_rate", type=float, default=0.005)
    ap.add_argument("--seed", type=int, default=1021)
    ap.add_argument("--batch_size", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=1)
    args = ap.parse_args(argv)

    device, flag, name = "cuda:0", "", args.model_name
    cols = ['click'] + SPARSE
    train = dict(load_h5_columns(args.h5, 'ctr_train' + args.postfix, cols))
    test = dict(load_h5_columns(args.h5, 'ctr_test' + args.postfix, cols))
    if int(np.min(train['301'])) == 0:                                              # scenario ids start at 1 (main.py:112-114)
        train['301'], test['301'] = np.asarray(train['301']) + 1, np.asarray(test['301']) + 1
    num_domains = max(len(np.unique(train[args.domain_col])), DATA_MAX[args.domain_col])          # main.py:131
    columns = [SparseFeat(f, vocabulary_size=int(DATA_MAX[f]) + 2, embedding_dim=args.embedding_dim) for f in SPARSE]
    names = get_feature_names(columns)
    batch_size, num_tasks = args.batch_size, num_domains
    if name == "xDeepFM":                                                           # main.py:220-221
        batch_size = 4096
    if name == "PNN":                                                               # main.py:244-250
        model = PNN(dnn_feature_columns=columns, seed=args.seed, device=device, domain_column=args.domain_col,
                    num_domains=num_domains, flag=flag)
    elif name == "AdaSparse":
        model = AdaSparse(linear_feature_columns=columns, dnn_feature_columns=columns, seed=args.seed, device=device,
                          domain_column=args.domain_col, num_domains=num_domains, flag=flag, domain_emb_dim=args.embedding_dim)
    elif name == "ESMM":
        num_tasks = 2
        model = ESMM(dnn_feature_columns=columns, seed=args.seed, device=device, task_types=['binary'] * 2,
                     task_names=['ctr0', 'ctr1'], domain_column=args.domain_col)
    elif name in MULTI_TASK:                                                        # main.py:262-265
        model = MODELS[name](dnn_feature_columns=columns, seed=args.seed, device=device, task_types=['binary'] * num_domains,
                             task_names=['ctr%d' % i for i in range(num_domains)], domain_column=args.domain_col, flag=flag)
    elif name != "Star_Net":                                                        # main.py:235-241
        model = MODELS[name](linear_feature_columns=columns, dnn_feature_columns=columns, seed=args.seed, device=device,
                             domain_column=args.domain_col, num_domains=num_domains, flag=flag)
    else:                                                                           # main.py:272-281
        model = Star_Net(linear_feature_columns=columns, dnn_feature_columns=columns, domain_column=args.domain_col,
                         num_domains=num_domains, domain_id_as_feature=True, dnn_hidden_units=(256, 128), use_domain_dnn=True,
                         use_domain_bn=True, seed=args.seed, device=device, flag=flag)
    loss = ["binary_crossentropy"] * num_tasks if name in MULTI_TASK else "binary_crossentropy"      # main.py:338-344
    model.compile(torch.optim.Adam(model.parameters(), lr=args.learning_rate), loss, metrics=["binary_crossentropy", "auc"])
    model.fit(x={f: train[f] for f in names}, y=np.asarray(train['click']), batch_size=batch_size, epochs=args.epochs, verbose=1)
    rep = model.evaluate_domains({f: test[f] for f in names}, np.asarray(test['click']), batch_size * 4, domain_col=args.domain_col)
    print("test AUC", round(rep["auc"], 4))
    for i in sorted(rep["domain_auc"]):
        print(f"Domain {i} test AUC", round(rep["domain_auc"][i], 4))
    print(f"{name}_{args.embedding_dim}_{args.learning_rate}_{args.seed}_{args.domain_col}_{flag}," +
          ",".join(str(round(a, 4)) for a in [rep["auc"]] + [rep["domain_auc"][i] for i in sorted(rep["domain_auc"])]) +
          "," + "%.6f" % rep["loss"])                                               # main.py:393


if __name__ == "__main__":
    main()
