"""What test_models_cpu.py and test_models_gpu.py share: the recorded cases of tests/golden/models/ (tools/gen_models_golden.py) and
the constructor calls that mirror the generator's."""
import functools
import os

import numpy as np
import torch

import satrans_amd as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")
CASES = ("wdl", "deepfm", "dcn_vector", "dcn_matrix", "mmoe", "star")
D, ROWS, BATCH, SCENARIOS, UNITS, L2, LR, EPOCHS = 16, 96, 32, 3, (16, 8), 1e-5, 1e-3, 2
LOSS_RTOL, PRED_ATOL, FWD_RTOL = 2e-5, 5e-4, 2e-5      # tests/test_gpu_parity.py's fit bounds; the sibling forward bound
CLASSES = {"wdl": S.WDL, "deepfm": S.DeepFM, "dcn_vector": S.DCN, "dcn_matrix": S.DCN, "mmoe": S.MMOE, "star": S.Star_Net}


@functools.lru_cache(maxsize=None)
def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def offset_of(name):
    return 1 if name in ("mmoe", "star") else 0


def columns(name, offset=None):
    offset = offset_of(name) if offset is None else offset
    vocab = {"dom": SCENARIOS + offset, "user": 50, "item": 37, "cate": 4}
    return [S.SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [S.DenseFeat("price", 1)]


def build(name, device="cpu", offset=None, **extra):
    cols = columns(name, offset)
    common = dict(l2_reg_embedding=L2, seed=7, device=device, flag="")
    common.update(extra)
    if name in ("wdl", "deepfm"):
        return CLASSES[name](cols, cols, dnn_hidden_units=UNITS, l2_reg_linear=L2, **common)
    if name.startswith("dcn"):
        return S.DCN(cols, cols, dnn_hidden_units=UNITS, l2_reg_linear=L2, cross_parameterization=name.split("_")[1], **common)
    if name == "mmoe":
        return S.MMOE(cols, expert_dnn_hidden_units=UNITS, gate_dnn_hidden_units=(8,), tower_dnn_hidden_units=(8,), l2_reg_linear=L2,
                      task_types=["binary"] * SCENARIOS, task_names=["ctr%d" % i for i in range(SCENARIOS)], domain_column="dom", **common)
    return S.Star_Net(cols, cols, "dom", SCENARIOS, True, dnn_hidden_units=UNITS, use_domain_dnn=True, use_domain_bn=True, **common)


def loss_arg(name):
    return ["binary_crossentropy"] * SCENARIOS if name == "mmoe" else "binary_crossentropy"


def inputs(name):
    c = load(name)
    return {k[2:]: c[k] for k in c if k.startswith("x/")}, c["y"]


def init_state(name):
    c = load(name)
    return {k[5:]: torch.from_numpy(c[k]) for k in c if k.startswith("init/")}
