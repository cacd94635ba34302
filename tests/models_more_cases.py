"""What test_models_more_cpu.py and test_models_more_gpu.py share: the ten further recorded cases of tests/golden/models/
(tools/gen_models_golden.py, MORE_CASES) and the constructor calls that mirror the generator's.  Shape and bounds are
tests/models_cases.py's."""
import functools
import os

import numpy as np
import torch

import satrans_amd as S
from tests.models_cases import BATCH, D, EPOCHS, FWD_RTOL, GOLDEN, L2, LOSS_RTOL, LR, PRED_ATOL, ROWS, UNITS  # noqa: F401

CASES = ("xdeepfm", "nfm", "afm", "autoint", "fibinet", "pnn", "adasparse", "sharedbottom", "ple", "esmm")
MULTI_TASK = ("sharedbottom", "ple", "esmm")
CLASSES = {"xdeepfm": S.xDeepFM, "nfm": S.NFM, "afm": S.AFM, "autoint": S.AutoInt, "fibinet": S.FiBiNET, "pnn": S.PNN,
           "adasparse": S.AdaSparse, "sharedbottom": S.SharedBottom, "ple": S.PLE, "esmm": S.ESMM}


def scenarios(name):
    return 2 if name == "esmm" else 3


@functools.lru_cache(maxsize=None)
def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def offset_of(name):
    return 1 if name in MULTI_TASK else 0


def columns(name):
    vocab = {"dom": scenarios(name) + offset_of(name), "user": 50, "item": 37, "cate": 4}
    return [S.SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [S.DenseFeat("price", 1)]


def build(name, device="cpu", **extra):
    cols = columns(name)
    common = dict(l2_reg_embedding=L2, seed=7, device=device, flag="")
    if name == "esmm":
        common.pop("flag")                                 # (esmm.py's constructor has none)
    common.update(extra)
    n = scenarios(name)
    tasks = dict(task_types=["binary"] * n, task_names=["ctr%d" % i for i in range(n)], domain_column="dom")
    if name == "xdeepfm":
        return S.xDeepFM(cols, cols, dnn_hidden_units=UNITS, cin_layer_size=(8, 8), l2_reg_linear=L2, **common)
    if name == "nfm":
        return S.NFM(cols, cols, dnn_hidden_units=UNITS, l2_reg_linear=L2, **common)
    if name == "afm":
        return S.AFM(cols, cols, attention_factor=4, l2_reg_linear=L2, **common)
    if name == "autoint":
        return S.AutoInt(cols, cols, att_layer_num=2, att_head_num=2, dnn_hidden_units=UNITS, **common)
    if name == "fibinet":
        return S.FiBiNET(cols, cols, dnn_hidden_units=UNITS, l2_reg_linear=L2, **common)
    if name == "pnn":
        return S.PNN(cols, dnn_hidden_units=UNITS, use_inner=True, use_outter=True, **common)
    if name == "adasparse":
        return S.AdaSparse(cols, cols, **{**dict(dnn_hidden_units=UNITS, l2_reg_linear=L2, domain_column="dom", num_domains=3,
                                                 domain_emb_dim=D), **common})
    if name == "sharedbottom":
        return S.SharedBottom(cols, **{**dict(bottom_dnn_hidden_units=UNITS, tower_dnn_hidden_units=(8,), l2_reg_linear=L2, **tasks),
                                       **common})
    if name == "ple":
        return S.PLE(cols, **{**dict(expert_dnn_hidden_units=UNITS, gate_dnn_hidden_units=(8,), tower_dnn_hidden_units=(8,),
                                     l2_reg_linear=L2, **tasks), **common})
    return S.ESMM(cols, **{**dict(tower_dnn_hidden_units=UNITS, l2_reg_linear=L2, **tasks), **common})


def loss_arg(name):
    return ["binary_crossentropy"] * scenarios(name) if name in MULTI_TASK else "binary_crossentropy"


def inputs(name):
    c = load(name)
    return {k[2:]: c[k] for k in c if k.startswith("x/")}, c["y"]


def init_state(name):
    c = load(name)
    return {k[5:]: torch.from_numpy(c[k]) for k in c if k.startswith("init/")}
