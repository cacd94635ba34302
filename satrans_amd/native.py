"""ctypes binding of libsatrans_hip.so (the C ABI declared in include/satrans_hip.h).

There is no CPU fallback: if the library cannot be loaded, or a call returns an error code, this
module raises.  Tensors cross the boundary as raw device pointers (`tensor.data_ptr()`) plus sizes;
the stream is torch's current HIP stream so that every kernel is ordered with the surrounding
torch plumbing (allocation, tiny scenario-encoder ops, RCCL collectives).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import torch

# HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); streams that share a queue serialise.  The
# data-parallel step runs five (launch stream, next-batch stream, tail stream, two RCCL communicator streams): on four queues
# its tail chains - gradient rows to their owners beside the slab reduction and the all-reduce - ran one after the other
# (measured, one rank through RCCL: 1.324 -> 1.214 ms/step with 8 queues; the one-GPU step is unchanged).  A default only: it has
# no effect when the caller's environment sets it, or when the HIP runtime was initialised before this import.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SATRANS_LIB_PATH") or os.path.join(_HERE, "libsatrans_hip.so")   # (override: kernel experiments)
ABI_VERSION = 7

ID_F32, ID_I32, ID_I64 = 0, 1, 2
META_Q, META_K, RELU_OUT, NO_RES, TRAIN, GATE, BILINEAR = 1, 2, 4, 8, 16, 32, 64
X_SORTED, Y_SORTED = 128, 256      # general path: activations stay in scenario-sorted order between the layers of a stack

_c_f32p = C.c_void_p
_vp = C.c_void_p


class LayerDesc(C.Structure):
    """Mirror of `satrans_layer_desc`."""
    _fields_ = [
        ("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("H", C.c_int32),
        ("U", C.c_int32), ("S", C.c_int32), ("flags", C.c_int32), ("layer", C.c_int32),
        ("drop_p", C.c_float), ("seed", C.c_uint32), ("step", C.c_uint32),
        ("tab_stride", C.c_int64),
        ("x", _vp), ("sid", _vp), ("order", _vp), ("seg", _vp),
        ("w_query", _vp), ("w_key", _vp), ("w_value", _vp), ("w_out", _vp),
        ("ln_g", _vp), ("ln_b", _vp),
        ("lnq_g", _vp), ("lnq_b", _vp), ("lnk_g", _vp), ("lnk_b", _vp),
        ("tab_q", _vp), ("tab_k", _vp),
        ("x_rows", _vp),
        ("attn_save", _vp),
    ]


class HeadDesc(C.Structure):
    """Mirror of `satrans_head_desc` (the head operands of satrans_layer_bwd_head)."""
    _fields_ = [("w", _vp), ("bias", _vp), ("labels", _vp), ("dense", _vp), ("dense_stride", C.c_int64),
                ("h_dense_cols", C.POINTER(C.c_int32)), ("n_dense", C.c_int32), ("loss_kind", C.c_int32),
                ("prob", _vp), ("logit", _vp), ("loss_sum", _vp), ("g_w", _vp), ("g_b", _vp), ("scratch", _vp)]


class LayerGrads(C.Structure):
    """Mirror of `satrans_layer_grads`."""
    _fields_ = [(k, _vp) for k in ("g_wq", "g_wk", "g_wv", "g_wo", "g_ln", "g_lnq", "g_lnk", "g_tab_q", "g_tab_k")]


class SelfAttDesc(C.Structure):
    """Mirror of `satrans_selfatt_desc`."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("flags", C.c_int32),
                ("layer", C.c_int32), ("drop_p", C.c_float), ("seed", C.c_uint32), ("step", C.c_uint32),
                ("x", _vp), ("w_query", _vp), ("w_key", _vp), ("w_value", _vp), ("w_res", _vp), ("ln_g", _vp), ("ln_b", _vp)]


class MetaNetDesc(C.Structure):
    """Mirror of `satrans_metanet_desc`."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("U", C.c_int32), ("S", C.c_int32), ("flags", C.c_int32),
                ("layer", C.c_int32), ("drop_p", C.c_float), ("seed", C.c_uint32), ("step", C.c_uint32),
                ("tab_stride", C.c_int64), ("x", _vp), ("order", _vp), ("seg", _vp), ("tab", _vp), ("ln_g", _vp), ("ln_b", _vp)]


class PNormDesc(C.Structure):
    """Mirror of `satrans_pnorm_desc`."""
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("S", C.c_int32), ("flags", C.c_int32), ("eps", C.c_float), ("factor", C.c_float),
                ("x", _vp), ("order", _vp), ("seg", _vp), ("weight", _vp), ("bias", _vp), ("shared_w", _vp), ("shared_b", _vp),
                ("running_mean", _vp), ("running_var", _vp)]


PNORM_ROW_CHUNK = 128      # SATRANS_PNORM_ROW_CHUNK: rows of one scenario's run that a workgroup of the reductions takes


STAR_ROW_TILE = 64           # SATRANS_STAR_ROW_TILE: rows of one scenario's run under a workgroup of the tower products
STAR_DW_ROW_CHUNK = 256      # SATRANS_STAR_DW_ROW_CHUNK: rows of a run that one partial of the weight gradients sums
STAR_MAX_LAYERS = 5          # SATRANS_STAR_MAX_LAYERS: up to 4 hidden layers and the logit layer


class StarDesc(C.Structure):
    """Mirror of `satrans_star_desc`."""
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("S", C.c_int32), ("L", C.c_int32), ("width", C.c_int32 * STAR_MAX_LAYERS),
                ("reserved", C.c_int32), ("x", _vp), ("order", _vp), ("seg", _vp),
                ("w_dom", _vp * STAR_MAX_LAYERS), ("b_dom", _vp * STAR_MAX_LAYERS), ("w_sh", _vp * STAR_MAX_LAYERS),
                ("b_sh", _vp * STAR_MAX_LAYERS)]


MMOE_ROW_TILE = 64           # SATRANS_MMOE_ROW_TILE: rows under a workgroup of the MMoE head's products
MMOE_DW_ROW_CHUNK = 256      # SATRANS_MMOE_DW_ROW_CHUNK: rows that one partial of its weight gradients sums
MMOE_MAX_EXPERTS = 8         # SATRANS_MMOE_MAX_EXPERTS
MMOE_MAX_HIDDEN = 3          # SATRANS_MMOE_MAX_HIDDEN: hidden layers of the expert, gate and tower DNNs, each


class MMoEDesc(C.Structure):
    """Mirror of `satrans_mmoe_desc`."""
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("E", C.c_int32), ("n_expert", C.c_int32),
                ("n_gate", C.c_int32), ("n_tower", C.c_int32), ("reserved", C.c_int32),
                ("expert_width", C.c_int32 * MMOE_MAX_HIDDEN), ("gate_width", C.c_int32 * MMOE_MAX_HIDDEN),
                ("tower_width", C.c_int32 * MMOE_MAX_HIDDEN), ("reserved2", C.c_int32),
                ("x", _vp), ("order", _vp), ("seg", _vp),
                ("expert_w", _vp * MMOE_MAX_HIDDEN), ("expert_b", _vp * MMOE_MAX_HIDDEN),
                ("gate_w", _vp * MMOE_MAX_HIDDEN), ("gate_b", _vp * MMOE_MAX_HIDDEN), ("gate_final_w", _vp),
                ("tower_w", _vp * MMOE_MAX_HIDDEN), ("tower_b", _vp * MMOE_MAX_HIDDEN), ("tower_final_w", _vp),
                ("out_bias", _vp)]


class MMoEGrads(C.Structure):
    """Mirror of `satrans_mmoe_grads`."""
    _fields_ = [("expert_w", _vp * MMOE_MAX_HIDDEN), ("expert_b", _vp * MMOE_MAX_HIDDEN),
                ("gate_w", _vp * MMOE_MAX_HIDDEN), ("gate_b", _vp * MMOE_MAX_HIDDEN), ("gate_final_w", _vp),
                ("tower_w", _vp * MMOE_MAX_HIDDEN), ("tower_b", _vp * MMOE_MAX_HIDDEN), ("tower_final_w", _vp),
                ("out_bias", _vp)]


PLE_ROW_TILE = 64              # SATRANS_PLE_ROW_TILE
PLE_DW_ROW_CHUNK = 256         # SATRANS_PLE_DW_ROW_CHUNK
PLE_MAX_OWN = 8                # SATRANS_PLE_MAX_OWN: specific + shared experts of one task's gate
PLE_MAX_SHARED_SCORES = 64     # SATRANS_PLE_MAX_SHARED_SCORES: T * specific + shared experts under the level-0 shared gate
PLE_MAX_HIDDEN = 3             # SATRANS_PLE_MAX_HIDDEN: hidden layers of the expert, gate and tower DNNs, each

# the parameter pointers of satrans_ple_desc / satrans_ple_grads in the header's order: (name, per hidden layer)
PLE_POINTERS = (("e0_w", True), ("e0_b", True), ("g0_w", True), ("g0_b", True), ("g0_final_w", False), ("sg0_w", True),
                ("sg0_b", True), ("sg0_final_w", False), ("spec_w", True), ("spec_b", True), ("shared_w", True), ("shared_b", True),
                ("gate_w", True), ("gate_b", True), ("gate_final_w", False), ("tower_w", True), ("tower_b", True),
                ("tower_final_w", False), ("out_bias", False))
_PLE_POINTER_FIELDS = [(name, _vp * PLE_MAX_HIDDEN if per_layer else _vp) for name, per_layer in PLE_POINTERS]


class PLEDesc(C.Structure):
    """Mirror of `satrans_ple_desc`."""
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("ns", C.c_int32), ("nsh", C.c_int32), ("levels", C.c_int32),
                ("n_expert", C.c_int32), ("n_gate", C.c_int32), ("n_tower", C.c_int32), ("reserved", C.c_int32),
                ("expert_width", C.c_int32 * PLE_MAX_HIDDEN), ("gate_width", C.c_int32 * PLE_MAX_HIDDEN),
                ("tower_width", C.c_int32 * PLE_MAX_HIDDEN), ("reserved2", C.c_int32),
                ("x", _vp), ("order", _vp), ("seg", _vp), ("task", _vp)] + _PLE_POINTER_FIELDS


class PLEGrads(C.Structure):
    """Mirror of `satrans_ple_grads`."""
    _fields_ = list(_PLE_POINTER_FIELDS)


# the parameter pointers of satrans_adasparse_desc / satrans_adasparse_grads in the header's order: (name, per layer)
ADASPARSE_POINTERS = (("lin_w", True), ("lin_b", True), ("prn_w", True), ("prn_b", True), ("final_w", False), ("out_bias", False))
_ADASPARSE_POINTER_FIELDS = [(name, _vp * MMOE_MAX_HIDDEN if per_layer else _vp) for name, per_layer in ADASPARSE_POINTERS]


class AdaSparseDesc(C.Structure):
    """Mirror of `satrans_adasparse_desc`."""
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("E", C.c_int32), ("n_layers", C.c_int32),
                ("width", C.c_int32 * MMOE_MAX_HIDDEN), ("alpha", C.c_float), ("beta", C.c_float), ("epsilon", C.c_float),
                ("x", _vp), ("emb", _vp)] + _ADASPARSE_POINTER_FIELDS


class AdaSparseGrads(C.Structure):
    """Mirror of `satrans_adasparse_grads`."""
    _fields_ = list(_ADASPARSE_POINTER_FIELDS)


# the parameter pointers of satrans_sharedbottom_desc / satrans_sharedbottom_grads in the header's order: (name, per hidden layer)
SHAREDBOTTOM_POINTERS = (("bottom_w", True), ("bottom_b", True), ("tower_w", True), ("tower_b", True), ("tower_final_w", False),
                         ("out_bias", False))
_SHAREDBOTTOM_POINTER_FIELDS = [(name, _vp * MMOE_MAX_HIDDEN if per_layer else _vp) for name, per_layer in SHAREDBOTTOM_POINTERS]


class SharedBottomDesc(C.Structure):
    """Mirror of `satrans_sharedbottom_desc` (row tile, chunk and layer limits are the MMoE head's: MMOE_*)."""
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("n_bottom", C.c_int32), ("n_tower", C.c_int32),
                ("reserved", C.c_int32), ("bottom_width", C.c_int32 * MMOE_MAX_HIDDEN), ("tower_width", C.c_int32 * MMOE_MAX_HIDDEN),
                ("x", _vp), ("order", _vp), ("seg", _vp)] + _SHAREDBOTTOM_POINTER_FIELDS


class SharedBottomGrads(C.Structure):
    """Mirror of `satrans_sharedbottom_grads`."""
    _fields_ = list(_SHAREDBOTTOM_POINTER_FIELDS)


CIN_MAX_LAYERS = 4            # SATRANS_CIN_MAX_LAYERS
CIN_MAX_FIELDS = 64           # SATRANS_CIN_MAX_FIELDS
CIN_MAX_WIDTH = 256           # SATRANS_CIN_MAX_WIDTH: channels of one layer
CIN_ROW_TILE = 64             # SATRANS_CIN_ROW_TILE: (sample, d) rows under a workgroup of the CIN products
CIN_DW_ROW_CHUNK = 1024       # SATRANS_CIN_DW_ROW_CHUNK: (sample, d) rows that one partial of its weight gradients sums


class CINDesc(C.Structure):
    """Mirror of `satrans_cin_desc`."""
    _fields_ = [("B", C.c_int32), ("M", C.c_int32), ("D", C.c_int32), ("L", C.c_int32), ("split_half", C.c_int32),
                ("reserved", C.c_int32), ("width", C.c_int32 * CIN_MAX_LAYERS), ("x0", _vp),
                ("w", _vp * CIN_MAX_LAYERS), ("b", _vp * CIN_MAX_LAYERS)]


class CINGrads(C.Structure):
    """Mirror of `satrans_cin_grads`."""
    _fields_ = [("w", _vp * CIN_MAX_LAYERS), ("b", _vp * CIN_MAX_LAYERS)]


CROSS_MAX_LAYERS = 8          # SATRANS_CROSS_MAX_LAYERS
CROSS_MAX_FEATURES = 4096     # SATRANS_CROSS_MAX_FEATURES: width of the cross network's rows
CROSS_VEC_ROW_CHUNK = 32      # SATRANS_CROSS_VEC_ROW_CHUNK: rows that one partial of the vector form's gradients sums


class CrossDesc(C.Structure):
    """Mirror of `satrans_cross_desc`."""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("L", C.c_int32), ("matrix", C.c_int32), ("x0", _vp), ("kernels", _vp),
                ("bias", _vp)]


class CrossGrads(C.Structure):
    """Mirror of `satrans_cross_grads`."""
    _fields_ = [("kernels", _vp), ("bias", _vp)]


FIBINET_MAX_FIELDS = 64          # SATRANS_FIBINET_MAX_FIELDS
FIBINET_MAX_DIM = 128            # SATRANS_FIBINET_MAX_DIM: the embedding size
FIBINET_DW_ROW_CHUNK = 256       # SATRANS_FIBINET_DW_ROW_CHUNK: rows that one partial of the bilinear weight gradients sums
FIBINET_SENET_ROW_CHUNK = 32     # SATRANS_FIBINET_SENET_ROW_CHUNK: rows that one partial of the excitation's gradients sums
BILINEAR_ALL, BILINEAR_EACH, BILINEAR_INTERACTION = 0, 1, 2      # SATRANS_BILINEAR_*
BILINEAR_TYPES = {"all": BILINEAR_ALL, "each": BILINEAR_EACH, "interaction": BILINEAR_INTERACTION}


class SENetDesc(C.Structure):
    """Mirror of `satrans_senet_desc`."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("R", C.c_int32), ("e", _vp), ("w1", _vp), ("w2", _vp)]


class SENetGrads(C.Structure):
    """Mirror of `satrans_senet_grads`."""
    _fields_ = [("w1", _vp), ("w2", _vp)]


class BilinearDesc(C.Structure):
    """Mirror of `satrans_bilinear_desc`."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("type", C.c_int32), ("e", _vp), ("w", _vp), ("a", _vp)]


# the parameter pointers of satrans_fibinet_desc / satrans_fibinet_grads in the header's order: (name, per hidden layer)
FIBINET_POINTERS = (("se_w1", False), ("se_w2", False), ("bilinear_w", False), ("dnn_w", True), ("dnn_b", True),
                    ("dnn_linear_w", False), ("out_bias", False))
_FIBINET_POINTER_FIELDS = [(name, _vp * MMOE_MAX_HIDDEN if per_layer else _vp) for name, per_layer in FIBINET_POINTERS]


class FiBiNETDesc(C.Structure):
    """Mirror of `satrans_fibinet_desc` (the DNN's layer limit is the MMoE head's: MMOE_MAX_HIDDEN)."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("type", C.c_int32), ("R", C.c_int32),
                ("dense_dim", C.c_int32), ("n_dnn", C.c_int32), ("reserved", C.c_int32), ("width", C.c_int32 * MMOE_MAX_HIDDEN),
                ("reserved2", C.c_int32), ("emb", _vp), ("dense", _vp)] + _FIBINET_POINTER_FIELDS


class FiBiNETGrads(C.Structure):
    """Mirror of `satrans_fibinet_grads`."""
    _fields_ = list(_FIBINET_POINTER_FIELDS)


PNN_MAX_FIELDS = 64              # SATRANS_PNN_MAX_FIELDS
PNN_MAX_DIM = 128                # SATRANS_PNN_MAX_DIM: the embedding size
PNN_DW_ROW_CHUNK = 256           # SATRANS_PNN_DW_ROW_CHUNK: rows that one partial of the outer product's kernel gradient sums
PNN_KERNEL_MAT, PNN_KERNEL_VEC, PNN_KERNEL_NUM = 0, 1, 2      # SATRANS_PNN_KERNEL_*
PNN_KERNEL_TYPES = {"mat": PNN_KERNEL_MAT, "vec": PNN_KERNEL_VEC, "num": PNN_KERNEL_NUM}


class InnerProductDesc(C.Structure):
    """Mirror of `satrans_inner_product_desc`."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("reserved", C.c_int32), ("e", _vp)]


class OuterProductDesc(C.Structure):
    """Mirror of `satrans_outer_product_desc`."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("kernel_type", C.c_int32), ("e", _vp), ("kernel", _vp)]


# the parameter pointers of satrans_pnn_desc / satrans_pnn_grads in the header's order: (name, per hidden layer)
PNN_POINTERS = (("kernel", False), ("dnn_w", True), ("dnn_b", True), ("dnn_linear_w", False), ("out_bias", False))
_PNN_POINTER_FIELDS = [(name, _vp * MMOE_MAX_HIDDEN if per_layer else _vp) for name, per_layer in PNN_POINTERS]


class PNNDesc(C.Structure):
    """Mirror of `satrans_pnn_desc` (the DNN's layer limit is the MMoE head's: MMOE_MAX_HIDDEN)."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("use_inner", C.c_int32), ("use_outer", C.c_int32),
                ("kernel_type", C.c_int32), ("dense_dim", C.c_int32), ("n_dnn", C.c_int32), ("width", C.c_int32 * MMOE_MAX_HIDDEN),
                ("reserved", C.c_int32), ("emb", _vp), ("dense", _vp)] + _PNN_POINTER_FIELDS


class PNNGrads(C.Structure):
    """Mirror of `satrans_pnn_grads`."""
    _fields_ = list(_PNN_POINTER_FIELDS)


FM_MAX_FIELDS = 64               # SATRANS_FM_MAX_FIELDS
FM_MAX_DIM = 128                 # SATRANS_FM_MAX_DIM: the embedding size
AFM_MAX_FACTOR = 64              # SATRANS_AFM_MAX_FACTOR: the attention factor A
AFM_MAX_WORKGROUPS = 1024        # SATRANS_AFM_MAX_WORKGROUPS: partials of AFM's parameter gradients at most
FMHEAD_DEEPFM, FMHEAD_NFM = 0, 1      # SATRANS_FMHEAD_*


class FMDesc(C.Structure):
    """Mirror of `satrans_fm_desc` (FM and BiInteractionPooling)."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("reserved", C.c_int32), ("e", _vp)]


# the parameter pointers of satrans_afm_desc / satrans_afm_grads in the header's order
AFM_POINTERS = ("attention_W", "attention_b", "projection_h", "projection_p")


class AFMDesc(C.Structure):
    """Mirror of `satrans_afm_desc`."""
    _fields_ = ([("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("A", C.c_int32), ("e", _vp)] +
                [(name, _vp) for name in AFM_POINTERS] + [("linear_logit", _vp), ("out_bias", _vp)])


class AFMGrads(C.Structure):
    """Mirror of `satrans_afm_grads`."""
    _fields_ = [(name, _vp) for name in AFM_POINTERS] + [("out_bias", _vp)]


# the parameter pointers of satrans_fmhead_desc / satrans_fmhead_grads in the header's order: (name, per hidden layer)
FMHEAD_POINTERS = (("dnn_w", True), ("dnn_b", True), ("dnn_linear_w", False), ("out_bias", False))
_FMHEAD_POINTER_FIELDS = [(name, _vp * MMOE_MAX_HIDDEN if per_layer else _vp) for name, per_layer in FMHEAD_POINTERS]


class FMHeadDesc(C.Structure):
    """Mirror of `satrans_fmhead_desc` (DeepFM's and NFM's heads; the DNN's layer limit is MMOE_MAX_HIDDEN)."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("kind", C.c_int32), ("use_fm", C.c_int32),
                ("dense_dim", C.c_int32), ("n_dnn", C.c_int32), ("reserved", C.c_int32), ("width", C.c_int32 * MMOE_MAX_HIDDEN),
                ("reserved2", C.c_int32), ("emb", _vp), ("dense", _vp), ("linear_logit", _vp)] + _FMHEAD_POINTER_FIELDS


class FMHeadGrads(C.Structure):
    """Mirror of `satrans_fmhead_grads`."""
    _fields_ = list(_FMHEAD_POINTER_FIELDS)


INTERACTING_MAX_WORKGROUPS = 512      # SATRANS_INTERACTING_MAX_WORKGROUPS: partials of a layer's weight gradients at most
AUTOINT_MAX_LAYERS = 8                # SATRANS_AUTOINT_MAX_LAYERS: interacting layers of a head at most
# the weight pointers of satrans_interacting_desc / satrans_autoint_desc in the header's order (deepctr's creation order)
INTERACTING_POINTERS = ("w_query", "w_key", "w_value", "w_res")


class InteractingDesc(C.Structure):
    """Mirror of `satrans_interacting_desc` (deepctr's InteractingLayer; flags: NO_RES, NO_SCALING)."""
    _fields_ = ([("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("flags", C.c_uint32),
                 ("reserved", C.c_int32), ("x", _vp)] + [(name, _vp) for name in INTERACTING_POINTERS])


# the DNN pointers of satrans_autoint_desc / satrans_autoint_grads in the header's order: (name, per hidden layer)
AUTOINT_POINTERS = (("dnn_w", True), ("dnn_b", True), ("dnn_linear_w", False), ("out_bias", False))
_AUTOINT_POINTER_FIELDS = [(name, _vp * MMOE_MAX_HIDDEN if per_layer else _vp) for name, per_layer in AUTOINT_POINTERS]


class AutoIntDesc(C.Structure):
    """Mirror of `satrans_autoint_desc` (the interacting stack, the DNN, dnn_linear and out.bias of AutoInt's head)."""
    _fields_ = ([("B", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("flags", C.c_uint32),
                 ("n_layers", C.c_int32), ("dense_dim", C.c_int32), ("n_dnn", C.c_int32), ("width", C.c_int32 * MMOE_MAX_HIDDEN),
                 ("reserved", C.c_int32), ("emb", _vp), ("dense", _vp)] +
                [(name, _vp * AUTOINT_MAX_LAYERS) for name in INTERACTING_POINTERS] + _AUTOINT_POINTER_FIELDS)


class AutoIntGrads(C.Structure):
    """Mirror of `satrans_autoint_grads`; int_w[l]: layer l's [3 or 4, D, D] block."""
    _fields_ = [("int_w", _vp * AUTOINT_MAX_LAYERS)] + list(_AUTOINT_POINTER_FIELDS)


# the parameter pointers of satrans_esmm_desc / satrans_esmm_grads in the header's order: (name, per hidden layer)
ESMM_POINTERS = (("dnn_w", True), ("dnn_b", True), ("final_w", False), ("out_bias", False))
_ESMM_POINTER_FIELDS = [(name, _vp * MMOE_MAX_HIDDEN if per_layer else _vp) for name, per_layer in ESMM_POINTERS]


class ESMMDesc(C.Structure):
    """Mirror of `satrans_esmm_desc` (ESMM's two towers, towers = 2, and WDL's DNN head, towers = 1; the layer limit is
    MMOE_MAX_HIDDEN; flags: TRAIN)."""
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("towers", C.c_int32), ("n_dnn", C.c_int32),
                ("width", C.c_int32 * MMOE_MAX_HIDDEN), ("flags", C.c_uint32), ("drop_p", C.c_float), ("seed", C.c_uint32),
                ("step", C.c_uint32), ("row_offset", C.c_uint32), ("x", _vp)] + _ESMM_POINTER_FIELDS


class ESMMGrads(C.Structure):
    """Mirror of `satrans_esmm_grads`."""
    _fields_ = list(_ESMM_POINTER_FIELDS)


class PoolField(C.Structure):
    """Mirror of `satrans_pool_field` (one field of the pooled gather; passed as a host array)."""
    _fields_ = [("col", C.c_int32), ("maxlen", C.c_int32), ("combiner", C.c_int32), ("len_col", C.c_int32),
                ("slot", C.c_int32), ("varlen", C.c_int32), ("lo", C.c_int64), ("hi", C.c_int64)]


POOL_COPY, POOL_SUM, POOL_MEAN, POOL_MAX = 0, 1, 2, 3      # satrans_pool_field.combiner (SATRANS_POOL_*)
POOL_MAX_LEN = 32                                           # SATRANS_POOL_MAX_LEN
POOL_MAX_FIELDS = 64                                        # SATRANS_POOL_MAX_FIELDS
# the launch grids of satrans_gather_fwd and satrans_pool_gather_fwd / satrans_pool_bwd (for tests that compute their trip counts)
GATHER_BLOCK, GATHER_ROWS_PER_THREAD, GATHER_MAX_BLOCKS = 256, 4, 2048      # SATRANS_GATHER_*
POOL_BLOCK, POOL_ITEMS, POOL_MAX_BLOCKS = 256, 4, 2048                      # SATRANS_POOL_BLOCK / _ITEMS / _MAX_BLOCKS


LINEAR_SAMPLES, LINEAR_MAX_BLOCKS = 16, 512      # SATRANS_LINEAR_SAMPLES / _MAX_BLOCKS: the grid of satrans_linear_fwd
LINEAR_SEG_CHUNK = 32                             # SATRANS_LINEAR_SEG_CHUNK: sorted positions per partial of the row gradients
LINEAR_DW_ROW_CHUNK = 64                          # SATRANS_LINEAR_DW_ROW_CHUNK: rows per partial of dweight


class LinearDesc(C.Structure):
    """Mirror of `satrans_linear_desc` (the order-1 term: 1-wide tables under the pooled gather's field table, and dense @ weight)."""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("R", C.c_int32), ("Fv", C.c_int32), ("id_dtype", C.c_int32),
                ("n_dense", C.c_int32), ("x_stride", C.c_int64), ("arena_rows", C.c_int64), ("dense_stride", C.c_int64),
                ("arena", _vp), ("fields", C.POINTER(PoolField)), ("X", _vp), ("dense", _vp), ("dense_cols", _vp), ("weight", _vp)]


class AdamHParams(C.Structure):
    """Mirror of `satrans_adam_hparams`."""
    _fields_ = [("lr_over_bc1", C.c_float), ("bc2_sqrt", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("l2", C.c_float), ("arith", C.c_int32)]


class AttnAtom(C.Structure):
    """Mirror of `satrans_attn_atom`."""
    _fields_ = [("q", C.c_int32), ("k", C.c_int32), ("thr", C.c_float)]


ATTN_MAX_RULES, ATTN_MAX_CLAUSES, ATTN_MAX_ATOMS, ATTN_MAX_HEADS = 8, 8, 4, 16      # SATRANS_ATTN_MAX_*


class AttnRule(C.Structure):
    """Mirror of `satrans_attn_rule` (a conjunction of clauses, each a disjunction of atoms att[h, b, q, k] > thr)."""
    _fields_ = [("n_clauses", C.c_int32), ("n_atoms", C.c_int32 * ATTN_MAX_CLAUSES),
                ("atoms", (AttnAtom * ATTN_MAX_ATOMS) * ATTN_MAX_CLAUSES)]


class AttnMatch(C.Structure):
    """Mirror of `satrans_attn_match` (16 bytes; numpy: ATTN_MATCH_DTYPE in attn_inst.py)."""
    _fields_ = [("index", C.c_int64), ("head", C.c_int32), ("rule", C.c_int32)]


ADAM_EXACT, ADAM_FAST = 0, 1      # satrans_adam_hparams.arith (SATRANS_ADAM_EXACT / SATRANS_ADAM_FAST)


# name -> (restype, argtypes); tests/test_host_cpu.py::test_library_exports_every_declared_symbol checks this table against the header
SIGNATURES = {
    "satrans_last_error": (C.c_char_p, []),
    "satrans_abi_version": (C.c_int, []),
    "satrans_stream_create_low_priority": (C.c_int, [C.POINTER(C.c_void_p)]),
    "satrans_stream_destroy": (C.c_int, [C.c_void_p]),
    "satrans_host_randperm": (C.c_int, [C.c_uint64, C.c_int64, _vp, _vp]),
    "satrans_kernel_timing": (C.c_int, [C.c_int]),
    "satrans_kernel_timing_read": (C.c_int, [_vp, _vp, C.c_int]),
    "satrans_bucket_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "satrans_bucket_scenarios": (C.c_int, [_vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                           _vp, C.c_int64, _vp]),
    "satrans_gather_fwd": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                     _vp, _vp]),
    "satrans_gather_read_probe_floats": (C.c_int64, []),
    "satrans_pool_argmax_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "satrans_pool_gather_fwd": (C.c_int, [_vp, C.c_int64, _vp, _vp, C.POINTER(PoolField), C.c_int, C.c_int, C.c_int, _vp, C.c_int,
                                          C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "satrans_pool_bwd": (C.c_int, [_vp, C.POINTER(PoolField), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "satrans_gather_read_probe": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp]),
    "satrans_linear_workspace_bytes": (C.c_int64, [C.POINTER(LinearDesc)]),
    "satrans_linear_fwd": (C.c_int, [C.POINTER(LinearDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "satrans_linear_bwd": (C.c_int, [C.POINTER(LinearDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "satrans_set_layer_impl": (C.c_int, [C.c_int]),
    "satrans_layer_fused_supported": (C.c_int, [C.POINTER(LayerDesc)]),
    "satrans_layer_fwd": (C.c_int, [C.POINTER(LayerDesc), _vp, _vp, _vp]),
"satrans_layer_fwd_bf16_supported": (C.c_int, [C.POINTER(LayerDesc)]),
    "satrans_layer_fwd_bf16": (C.c_int, [C.POINTER(LayerDesc), _vp, _vp]),
    "satrans_stack_fwd_bf16_supported": (C.c_int, [C.c_int, C.POINTER(C.POINTER(LayerDesc))]),
    "satrans_stack_fwd_bf16": (C.c_int, [C.c_int, C.POINTER(C.POINTER(LayerDesc)), _vp, _vp]),
    "satrans_stack_fwd_bf16_head": (C.c_int, [C.c_int, C.POINTER(C.POINTER(LayerDesc)), C.POINTER(HeadDesc), _vp]),
"satrans_layer_generic_supported": (C.c_int, [C.POINTER(LayerDesc)]),
    "satrans_layer_generic_saved_floats": (C.c_int64, [C.POINTER(LayerDesc)]),
    "satrans_layer_generic_scratch_floats": (C.c_int64, [C.POINTER(LayerDesc)]),
    "satrans_layer_fwd_generic": (C.c_int, [C.POINTER(LayerDesc), _vp, _vp, _vp, _vp]),
    "satrans_layer_bwd_generic": (C.c_int, [C.POINTER(LayerDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _vp]),
    "satrans_set_generic_attention": (C.c_int, [C.c_int]),
"satrans_selfatt_saved_floats": (C.c_int64, [C.POINTER(SelfAttDesc)]),
    "satrans_selfatt_scratch_floats": (C.c_int64, [C.POINTER(SelfAttDesc)]),
    "satrans_selfatt_fwd": (C.c_int, [C.POINTER(SelfAttDesc), _vp, _vp, _vp, _vp]),
    "satrans_selfatt_bwd": (C.c_int, [C.POINTER(SelfAttDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "satrans_metanet_saved_floats": (C.c_int64, [C.POINTER(MetaNetDesc)]),
    "satrans_metanet_scratch_floats": (C.c_int64, [C.POINTER(MetaNetDesc)]),
    "satrans_metanet_fwd": (C.c_int, [C.POINTER(MetaNetDesc), _vp, _vp, _vp]),
    "satrans_metanet_bwd": (C.c_int, [C.POINTER(MetaNetDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "satrans_pnorm_saved_floats": (C.c_int64, [C.POINTER(PNormDesc)]),
    "satrans_pnorm_workspace_floats": (C.c_int64, [C.POINTER(PNormDesc)]),
    "satrans_pnorm_fwd": (C.c_int, [C.POINTER(PNormDesc), _vp, _vp, _vp, _vp]),
    "satrans_pnorm_bwd": (C.c_int, [C.POINTER(PNormDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "satrans_star_saved_floats": (C.c_int64, [C.POINTER(StarDesc)]),
    "satrans_star_workspace_floats": (C.c_int64, [C.POINTER(StarDesc)]),
    "satrans_star_fwd": (C.c_int, [C.POINTER(StarDesc), _vp, _vp, _vp]),
    "satrans_star_bwd": (C.c_int, [C.POINTER(StarDesc), _vp, _vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                   C.POINTER(_vp), _vp]),
    "satrans_mmoe_saved_floats": (C.c_int64, [C.POINTER(MMoEDesc)]),
    "satrans_mmoe_workspace_floats": (C.c_int64, [C.POINTER(MMoEDesc)]),
    "satrans_mmoe_fwd": (C.c_int, [C.POINTER(MMoEDesc), _vp, _vp, _vp]),
    "satrans_mmoe_bwd": (C.c_int, [C.POINTER(MMoEDesc), _vp, _vp, _vp, _vp, C.POINTER(MMoEGrads), _vp]),
    "satrans_ple_saved_floats": (C.c_int64, [C.POINTER(PLEDesc)]),
    "satrans_ple_workspace_floats": (C.c_int64, [C.POINTER(PLEDesc)]),
    "satrans_ple_fwd": (C.c_int, [C.POINTER(PLEDesc), _vp, _vp, _vp]),
    "satrans_ple_bwd": (C.c_int, [C.POINTER(PLEDesc), _vp, _vp, _vp, _vp, C.POINTER(PLEGrads), _vp]),
    "satrans_adasparse_saved_floats": (C.c_int64, [C.POINTER(AdaSparseDesc)]),
    "satrans_adasparse_workspace_floats": (C.c_int64, [C.POINTER(AdaSparseDesc)]),
    "satrans_adasparse_fwd": (C.c_int, [C.POINTER(AdaSparseDesc), _vp, _vp, _vp]),
    "satrans_adasparse_bwd": (C.c_int, [C.POINTER(AdaSparseDesc), _vp, _vp, _vp, _vp, _vp, C.POINTER(AdaSparseGrads), _vp]),
    "satrans_adasparse_set_forward": (C.c_int, [C.c_int]),
    "satrans_sharedbottom_saved_floats": (C.c_int64, [C.POINTER(SharedBottomDesc)]),
    "satrans_sharedbottom_workspace_floats": (C.c_int64, [C.POINTER(SharedBottomDesc)]),
    "satrans_sharedbottom_fwd": (C.c_int, [C.POINTER(SharedBottomDesc), _vp, _vp, _vp]),
    "satrans_sharedbottom_bwd": (C.c_int, [C.POINTER(SharedBottomDesc), _vp, _vp, _vp, _vp, C.POINTER(SharedBottomGrads), _vp]),
    "satrans_sharedbottom_set_forward": (C.c_int, [C.c_int]),
    "satrans_cin_saved_floats": (C.c_int64, [C.POINTER(CINDesc)]),
    "satrans_cin_workspace_floats": (C.c_int64, [C.POINTER(CINDesc)]),
    "satrans_cin_fwd": (C.c_int, [C.POINTER(CINDesc), _vp, _vp, _vp]),
    "satrans_cin_bwd": (C.c_int, [C.POINTER(CINDesc), _vp, _vp, _vp, _vp, C.POINTER(CINGrads), _vp]),
    "satrans_cross_saved_floats": (C.c_int64, [C.POINTER(CrossDesc)]),
    "satrans_cross_workspace_floats": (C.c_int64, [C.POINTER(CrossDesc)]),
    "satrans_cross_fwd": (C.c_int, [C.POINTER(CrossDesc), _vp, _vp, _vp]),
    "satrans_cross_bwd": (C.c_int, [C.POINTER(CrossDesc), _vp, _vp, _vp, _vp, C.POINTER(CrossGrads), _vp]),
    "satrans_senet_saved_floats": (C.c_int64, [C.POINTER(SENetDesc)]),
    "satrans_senet_workspace_floats": (C.c_int64, [C.POINTER(SENetDesc)]),
    "satrans_senet_fwd": (C.c_int, [C.POINTER(SENetDesc), _vp, _vp, _vp]),
    "satrans_senet_bwd": (C.c_int, [C.POINTER(SENetDesc), _vp, _vp, _vp, _vp, _vp, C.POINTER(SENetGrads), _vp]),
    "satrans_bilinear_workspace_floats": (C.c_int64, [C.POINTER(BilinearDesc)]),
    "satrans_bilinear_fwd": (C.c_int, [C.POINTER(BilinearDesc), _vp, _vp]),
    "satrans_bilinear_bwd": (C.c_int, [C.POINTER(BilinearDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "satrans_fibinet_saved_floats": (C.c_int64, [C.POINTER(FiBiNETDesc)]),
    "satrans_fibinet_workspace_floats": (C.c_int64, [C.POINTER(FiBiNETDesc)]),
    "satrans_fibinet_fwd": (C.c_int, [C.POINTER(FiBiNETDesc), _vp, _vp, _vp]),
    "satrans_fibinet_bwd": (C.c_int, [C.POINTER(FiBiNETDesc), _vp, _vp, _vp, _vp, _vp, C.POINTER(FiBiNETGrads), _vp]),
    "satrans_inner_product_fwd": (C.c_int, [C.POINTER(InnerProductDesc), _vp, _vp]),
    "satrans_inner_product_bwd": (C.c_int, [C.POINTER(InnerProductDesc), _vp, _vp, _vp]),
    "satrans_outer_product_workspace_floats": (C.c_int64, [C.POINTER(OuterProductDesc)]),
    "satrans_outer_product_fwd": (C.c_int, [C.POINTER(OuterProductDesc), _vp, _vp]),
    "satrans_outer_product_bwd": (C.c_int, [C.POINTER(OuterProductDesc), _vp, _vp, _vp, _vp, _vp]),
    "satrans_pnn_saved_floats": (C.c_int64, [C.POINTER(PNNDesc)]),
    "satrans_pnn_workspace_floats": (C.c_int64, [C.POINTER(PNNDesc)]),
    "satrans_pnn_fwd": (C.c_int, [C.POINTER(PNNDesc), _vp, _vp, _vp]),
    "satrans_pnn_bwd": (C.c_int, [C.POINTER(PNNDesc), _vp, _vp, _vp, _vp, _vp, C.POINTER(PNNGrads), _vp]),
    "satrans_fm_fwd": (C.c_int, [C.POINTER(FMDesc), _vp, _vp]),
    "satrans_fm_bwd": (C.c_int, [C.POINTER(FMDesc), _vp, _vp, _vp]),
    "satrans_bipool_fwd": (C.c_int, [C.POINTER(FMDesc), _vp, _vp]),
    "satrans_bipool_bwd": (C.c_int, [C.POINTER(FMDesc), _vp, _vp, _vp]),
    "satrans_afm_saved_floats": (C.c_int64, [C.POINTER(AFMDesc)]),
    "satrans_afm_workspace_floats": (C.c_int64, [C.POINTER(AFMDesc)]),
    "satrans_afm_fwd": (C.c_int, [C.POINTER(AFMDesc), _vp, _vp, _vp]),
    "satrans_afm_bwd": (C.c_int, [C.POINTER(AFMDesc), _vp, _vp, _vp, _vp, C.POINTER(AFMGrads), _vp]),
    "satrans_fmhead_saved_floats": (C.c_int64, [C.POINTER(FMHeadDesc)]),
    "satrans_fmhead_workspace_floats": (C.c_int64, [C.POINTER(FMHeadDesc)]),
    "satrans_fmhead_fwd": (C.c_int, [C.POINTER(FMHeadDesc), _vp, _vp, _vp]),
    "satrans_fmhead_bwd": (C.c_int, [C.POINTER(FMHeadDesc), _vp, _vp, _vp, _vp, _vp, C.POINTER(FMHeadGrads), _vp]),
    "satrans_interacting_saved_floats": (C.c_int64, [C.POINTER(InteractingDesc)]),
    "satrans_interacting_scratch_floats": (C.c_int64, [C.POINTER(InteractingDesc)]),
    "satrans_interacting_fwd": (C.c_int, [C.POINTER(InteractingDesc), _vp, _vp, _vp, _vp]),
    "satrans_interacting_bwd": (C.c_int, [C.POINTER(InteractingDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "satrans_autoint_saved_floats": (C.c_int64, [C.POINTER(AutoIntDesc)]),
    "satrans_autoint_workspace_floats": (C.c_int64, [C.POINTER(AutoIntDesc)]),
    "satrans_autoint_fwd": (C.c_int, [C.POINTER(AutoIntDesc), _vp, C.POINTER(_vp), _vp, _vp]),
    "satrans_autoint_bwd": (C.c_int, [C.POINTER(AutoIntDesc), _vp, _vp, _vp, _vp, _vp, C.POINTER(AutoIntGrads), _vp]),
    "satrans_esmm_saved_floats": (C.c_int64, [C.POINTER(ESMMDesc)]),
    "satrans_esmm_workspace_floats": (C.c_int64, [C.POINTER(ESMMDesc)]),
    "satrans_esmm_fwd": (C.c_int, [C.POINTER(ESMMDesc), _vp, _vp, _vp]),
    "satrans_esmm_bwd": (C.c_int, [C.POINTER(ESMMDesc), _vp, _vp, _vp, _vp, C.POINTER(ESMMGrads), _vp]),
    "satrans_esmm_set_forward": (C.c_int, [C.c_int]),
    "satrans_layer_bwd_slab_floats": (C.c_int64, [C.POINTER(LayerDesc)]),
    "satrans_layer_attn_save_floats": (C.c_int64, [C.POINTER(LayerDesc)]),
    "satrans_batch_metrics": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "satrans_layer_bwd": (C.c_int, [C.POINTER(LayerDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp]),
    "satrans_layer_bwd_head_supported": (C.c_int, [C.POINTER(LayerDesc), C.POINTER(HeadDesc)]),
    "satrans_layer_bwd_head_scratch_floats": (C.c_int64, [C.POINTER(LayerDesc), C.c_int]),
    "satrans_layer_bwd_head": (C.c_int, [C.POINTER(LayerDesc), C.POINTER(HeadDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp]),
    "satrans_layer_bwd_deferred_supported": (C.c_int, [C.POINTER(LayerDesc)]),
    "satrans_layer_bwd_launch": (C.c_int, [C.POINTER(LayerDesc), _vp, _vp, _vp, _vp]),
    "satrans_layer_bwd_head_launch": (C.c_int, [C.POINTER(LayerDesc), C.POINTER(HeadDesc), _vp, _vp, _vp]),
    "satrans_layer_bwd_reduce": (C.c_int, [C.c_int, C.POINTER(C.POINTER(LayerDesc)), C.POINTER(_vp), C.POINTER(LayerGrads),
                                           C.POINTER(HeadDesc), _vp]),
    "satrans_head_scratch_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "satrans_head": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp]),
"satrans_head_loss": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "satrans_point_loss_partials": (C.c_int64, [C.c_int]),
    "satrans_point_loss": (C.c_int, [_vp, C.c_int64, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "satrans_point_loss_routed": (C.c_int, [_vp, C.c_int64, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "satrans_optim_flat": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int64, C.c_float, C.c_float, C.c_float, _vp]),
    "satrans_adam_flat": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.POINTER(AdamHParams), _vp]),
    "satrans_adam_flat_sum": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.POINTER(AdamHParams), _vp, C.c_int64, _vp, _vp]),
    "satrans_embed_sort_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "satrans_embed_sort": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp]),
    "satrans_embed_reg_partials": (C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    "satrans_embed_partial_ws_floats": (C.c_int64, [C.c_int64, C.c_int]),
    "satrans_scenario_table_fwd": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "satrans_scenario_table_bwd_ws_floats": (C.c_int64, [C.c_int, C.c_int]),
    "satrans_scenario_table_bwd": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "satrans_scenario_inputs_fwd": (C.c_int, [C.POINTER(_vp), _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, _vp]),
    "satrans_scenario_inputs_bwd": (C.c_int, [C.POINTER(_vp), C.POINTER(C.c_int32), _vp, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                              _vp, C.c_int, _vp]),
    "satrans_scenario_relu_fwd": (C.c_int, [_vp, C.c_int64, _vp, _vp]),
    "satrans_scenario_relu_bwd": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp]),
    "satrans_embed_adam_touched": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int64, _vp, _vp,
                                             C.POINTER(AdamHParams), _vp, _vp, C.c_int, _vp]),
    "satrans_embed_adam_untouched": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, C.POINTER(AdamHParams),
                                               _vp, C.c_int, _vp]),
    "satrans_embed_mark_touched": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    "satrans_embed_segment_sums": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "satrans_embed_adam_rows_partials": (C.c_int64, [C.c_int64, C.c_int]),
    "satrans_embed_adam_rows": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, C.POINTER(AdamHParams),
                                          C.c_int, _vp, _vp]),
    "satrans_embed_pack_rows": (C.c_int, [_vp, C.c_int64, _vp, C.c_int, _vp, _vp]),
    "satrans_embed_rows_sort_fields": (C.c_int, [_vp, C.c_int, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp, _vp]),
    "satrans_embed_merge_runs": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int64), C.c_int, _vp, _vp, _vp]),
    "satrans_embed_inverse_positions": (C.c_int, [_vp, C.c_int64, _vp, _vp]),
    "satrans_embed_sort_fields": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            _vp, _vp, _vp]),
    "satrans_embed_lazy_reg_partials": (C.c_int64, [C.c_int64, C.c_int]),
    "satrans_embed_lazy_replay": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int64, C.c_int, _vp,
                                            C.POINTER(AdamHParams), _vp, _vp]),
    "satrans_embed_lazy_flush": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int, C.c_int, _vp, C.POINTER(AdamHParams),
                                           C.c_int64, _vp, _vp]),
    "satrans_embed_lazy_replay_reg64": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int64, C.c_int, _vp,
                                                  C.POINTER(AdamHParams), _vp, _vp]),
    "satrans_embed_lazy_flush_reg64": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int, C.c_int, _vp, C.POINTER(AdamHParams),
                                                 C.c_int64, _vp, _vp]),
    "satrans_embed_lazy_mark": (C.c_int, [_vp, C.c_int64, _vp, C.c_int, _vp]),
    "satrans_embed1_lazy_replay": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(PoolField), C.c_int, C.c_int,
                                             _vp, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, C.POINTER(AdamHParams), _vp]),
    "satrans_embed1_adam_rows": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(AdamHParams), C.c_int,
                                           _vp]),
    "satrans_embed1_lazy_flush": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, C.POINTER(AdamHParams), _vp]),
    "satrans_debug_check_packed_math": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    "satrans_embed_grad_dense": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int, C.c_float, _vp, _vp]),
    "satrans_sum_f64": (C.c_int, [_vp, C.c_int64, _vp, C.c_int, _vp]),
    "satrans_attn_stats_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "satrans_attn_stats_accumulate": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int64, _vp]),
    "satrans_attn_inst_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "satrans_attn_inst_check_rules": (C.c_int, [C.POINTER(AttnRule), C.c_int, C.c_int]),
    "satrans_attn_inst_match": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(AttnRule), C.c_int, _vp, C.c_int64, _vp,
                                          C.c_int64, _vp, _vp, _vp, C.c_int64, _vp]),
    "satrans_attn_inst_gather": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, _vp, _vp,
                                           _vp, _vp, C.c_int64, C.c_int, _vp, _vp]),
}

_lib: Optional[C.CDLL] = None


class NativeError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU).  Returns the .so path."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    if force:
        for f in os.listdir(os.path.join(_HERE, "csrc", "build")) if os.path.isdir(os.path.join(_HERE, "csrc", "build")) else []:
            os.remove(os.path.join(_HERE, "csrc", "build", f))
    subprocess.run(["bash", script], check=True)
    return LIB_PATH


def source_hash() -> str:
    """sha256 over the kernel sources the library is built from (csrc/*.hip, csrc/*.h, include/*.h; names and bytes, sorted).
    Profiles under profiles/ record it, so a counter summary can be matched to the code it was taken on - the hash of the
    .so would differ between two builds of identical sources."""
    import hashlib
    h = hashlib.sha256()
    inc = os.path.join(os.path.dirname(_HERE), "include")
    files = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc")) if f.endswith((".hip", ".h"))]
    files += [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")]
    for path in sorted(files, key=os.path.basename):
        h.update(os.path.basename(path).encode() + b"\0")
        h.update(open(path, "rb").read())
    return h.hexdigest()


def lib() -> C.CDLL:
    """Load (once) and type the shared library.  Raises NativeError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} is missing: the SATrans hot path has no CPU/eager fallback. "
            f"Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `bash satrans_amd/csrc/build.sh`.")
    try:
        handle = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the box
        raise NativeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise NativeError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype, fn.argtypes = res, args
    if handle.satrans_abi_version() != ABI_VERSION:
        raise NativeError(f"ABI version mismatch: library {handle.satrans_abi_version()}, binding {ABI_VERSION}")
    _lib = handle
    return handle


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().satrans_last_error()
        raise NativeError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a contiguous tensor (None stays NULL)."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise NativeError("non-contiguous tensor handed to the native library")
    return t.data_ptr()


def stream_handle(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise NativeError(
            f"{what}: tensor is on '{t.device}'. The SATrans hot path runs only as HIP kernels on an MI355X; "
            f"construct the model with device='cuda:0' (there is no CPU fallback; the CPU restatement lives in "
            f"oracle/ and is test infrastructure).")


def id_dtype_of(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return ID_F32
    if t.dtype == torch.int32:
        return ID_I32
    if t.dtype == torch.int64:
        return ID_I64
    raise NativeError(f"input matrix dtype {t.dtype} is not one of float32/int32/int64")
