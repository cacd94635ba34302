"""Sibling users of the attention-path kernels, for the reference's baselines that plug them in.

  * `SelfAttention_Layer` - reference models/submodules.py:178-238 (`usetrans` in models/star.py:70-72, mmoe.py:77-79,
    ple.py:72-74, sharedbottom.py:65-67, adasparse.py:145-147): same constructor, same parameter creation order and init
    (W_Query, W_Key, W_Value, W_Out, layer_norm, W_Res ~ N(0, 0.05); W_Out is never used by the reference's forward either).
  * `MetaTransformation` - reference BaseModel.meta_transformation (models/basemodel.py:191-199) with its MetaNet
    (models/submodules.py:64-103): the scenario embedding, the one-Linear scenario encoder and the MetaNet over the embedding
    block.  The generated weights are tabulated per SCENARIO ([S,P], S rows) instead of per sample ([B,P]).

  * `MDR_BatchNorm` - reference models/submodules.py:107-175, the partitioned normalisation of STAR (`use_domain_bn` in
    models/star.py:81-82,147-154): same constructor, parameters, buffers and state_dict keys; and `PartitionedNorm`, the
    ModuleList of them that star.py loops over, as ONE pass over all scenarios (csrc/pnorm.hip).

  * `StarTowers` - STAR's star-topology FC towers (models/star.py:156-170: per-scenario weight * shared weight, applied to each
    scenario's rows) for a mixed batch (csrc/star.hip), and `StarHead`, the scenario-dependent half of `Star_Net.forward`
    (star.py:144-173): the partitioned normalisation, then the towers, on one bucketing of the batch.

  * `MMoEHead` - the expert / gate / tower half of the reference's MMOE.forward (models/mmoe.py:142-171) for a mixed batch
    under the one-task-per-scenario loss of mtl_basemodel.py:268-269: the experts over all rows, each row through its own
    task's gate, mixture, tower and logit only (csrc/mmoe.hip).

  * `PLEHead` - the expert / gate / tower half of the reference's PLE.forward (models/ple.py:161-248), one or two CGC levels,
    for a mixed batch under the same loss: what a row's own task needs is routed, what the shared mixture needs stays dense
    (csrc/ple.hip).

  * `PrunedDNN` - the reference's DNN_w_Pruner (models/adasparse.py:28-106): every layer's output times a scenario-aware
    pruning factor cut to exactly zero below a threshold, both products of a layer in one launch; and `AdaSparseHead`, the
    part of AdaSparse.forward behind the embeddings (adasparse.py:185-189).  Nothing is routed here (csrc/adasparse.hip).

  * `CIN` - deepctr's compressed interaction network, which the reference's xDeepFM calls (models/xdeepfm.py:73,96-98), with
    the outer product as a generated operand of the products (csrc/cin.hip); and `XDeepFMHead`, the part of xDeepFM.forward
    behind the embeddings (xdeepfm.py:94-115).  Single-task: nothing is routed.

  * `CrossNet` - deepctr's cross network in its vector and matrix forms, which the reference's DCN calls (models/dcn.py:70,101):
    the vector form one launch for the whole stack, the matrix form a tile product per layer (csrc/cross.hip); and `DCNHead`,
    the part of DCN.forward behind the embeddings (dcn.py:90-113).

  * `SENETLayer` and `BilinearInteraction` - deepctr's two FiBiNET layers, which the reference's FiBiNET calls
    (models/fibinet.py:51-52,93-95): the excitation a wave per row, all pairs' bilinear products in one launch; and
    `FiBiNETHead`, the part of FiBiNET.forward behind the embeddings (fibinet.py:91-112) with its DNN on the dense layer launcher
    of csrc/head_layers.h, the whole head one autograd.Function (csrc/fibinet.hip).

  * `InnerProductLayer` and `OutterProductLayer` - deepctr's two PNN layers, which the reference's PNN calls
    (models/pnn.py:61,65,94-99): a row read once for all of its inner, 'vec' and 'num' products, the 'mat' outer product one
    D x D product per pair on the matrix pipe reduced inside the workgroup; and `PNNHead`, the part of PNN.forward behind the
    embeddings (pnn.py:91-114), the whole head one autograd.Function (csrc/pnn.hip).

  * `FM`, `BiInteractionPooling` and `AFMLayer` - deepctr's pairwise-interaction layers, which the reference's DeepFM, NFM and AFM
    call (models/deepfm.py:57, nfm.py:56, afm.py:47): FM and the pooling one pass over the rows each way; AFM with a sample's rows
    staged once, the pair products, the scores, the softmax and the relu mask kept on chip - none of deepctr's [B, P, D] tensors
    exists; and `DeepFMHead`, `NFMHead` and `AFMHead`, the parts of the three forwards behind the embeddings (deepfm.py:87-113,
    nfm.py:73-83, afm.py:66-73) with linear_logit and out.bias, each head one autograd.Function (csrc/fm.hip).

  * `InteractingLayer` - deepctr's interacting layer, which the reference's AutoInt stacks (models/autoint.py:13,75-76; NOT
    SelfAttention_Layer: W_Query, W_key, W_Value, W_Res only, scaling off by default, relu(o + x W_Res) as the tail): one launch
    forward, one plus an ordered reduce backward, whole samples held on chip, only the softmax rows' (max, sum) saved; and
    `AutoIntHead`, the part of AutoInt.forward behind the embeddings (autoint.py:93-121), the whole head one autograd.Function
    (csrc/autoint.hip).

  * `ESMMHead` - the two towers, sigmoids and product of the reference's ESMM.forward (models/esmm.py:84-96), and `WDLHead`, the
    DNN half of WDL.forward (models/wdl.py:75-77): the same kernels at two towers and at one, with dropout inside the DNNs as a
    compile-time option of the dense layer launcher of csrc/head_layers.h, each head one autograd.Function (csrc/esmm.hip).

  * `LinearModel` - deepctr's `Linear`, the order-1 term `linear_model(X)` of the reference's baselines (models/meta_basemodel.py:
    34-92): 1-wide tables under the pooled gather's field table plus dense @ weight, one launch forward in a fixed summation
    order, an ordered segment sum without float atomics backward (csrc/linear.hip); and `FeatureEmbedding`, the reference's
    `input_from_feature_columns` (meta_basemodel.py:519-545) as one autograd.Function over the existing gather / pool / sort
    ABI (csrc/gather.hip, csrc/pool.hip, csrc/embed_adam.hip).  Together they turn `X` into the `linear_logit`, `emb` and `dense`
    that every head above starts from, with dense table gradients for any torch optimizer - or, adopted by optim.TableAdam, the
    engine's touched-rows lazy Adam step with no dense gradient at all.

All are ordinary `nn.Module`s whose forward/backward are HIP launches (csrc/layer_generic.hip, csrc/pnorm.hip, csrc/star.hip,
csrc/mmoe.hip, csrc/ple.hip, csrc/adasparse.hip, csrc/cin.hip, csrc/cross.hip, csrc/fibinet.hip, csrc/pnn.hip, csrc/fm.hip,
csrc/autoint.hip, csrc/esmm.hip, csrc/linear.hip) wrapped
in a
`torch.autograd.Function`, so they can sit inside any torch model.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _NormBase

from . import native as N
from .basemodel import _LinearTables, make_embedding_tables

NO_SCALING, NO_NORM = 128, 256


class _DropClock:
    """Counter-based dropout needs a (seed, step) pair per forward; the step advances with every training forward."""

    def __init__(self):
        self.seed = int(torch.initial_seed() & 0xFFFFFFFF)
        self.step = 0


class _SelfAttFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wq, wk, wv, wres, ln_w, ln_b, mod):
        lib = N.lib()
        N.require_gpu(x, "SelfAttention_Layer")
        x = x.contiguous().float()
        B, F, D = x.shape
        d = N.SelfAttDesc()
        d.B, d.F, d.D, d.H = B, F, D, mod.head_num
        d.flags = (N.TRAIN if mod.training else 0) | (0 if mod.use_res else N.NO_RES) | (0 if mod.scaling else NO_SCALING)
        d.layer, d.drop_p = 0, 0.1
        if mod.training:
            mod._clock.step += 1
        d.seed, d.step = mod._clock.seed, mod._clock.step & 0xFFFFFFFF
        ln = torch.cat([ln_w.detach().reshape(-1), ln_b.detach().reshape(-1)]).contiguous()
        d.x, d.w_query, d.w_key, d.w_value = x.data_ptr(), wq.data_ptr(), wk.data_ptr(), wv.data_ptr()
        d.w_res = wres.data_ptr() if wres is not None else None
        d.ln_g, d.ln_b = ln.data_ptr(), ln.data_ptr() + 4 * D
        n = int(lib.satrans_selfatt_saved_floats(C.byref(d)))
        if n < 0:
            raise N.NativeError(f"SelfAttention_Layer: shape B={B} F={F} D={D} H={mod.head_num} is not supported")
        saved = torch.empty(n, dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        att = None
        if mod.capture_attention:
            att = torch.empty(mod.head_num, B, F, F, dtype=torch.float32, device=x.device)
        N.check(lib.satrans_selfatt_fwd(C.byref(d), y.data_ptr(), att.data_ptr() if att is not None else None, saved.data_ptr(),
                                        N.stream_handle(x.device)), "satrans_selfatt_fwd")
        mod.normalized_att_scores = att
        ctx.desc, ctx.mod = d, mod
        ctx.save_for_backward(x, wq, wk, wv, wres if wres is not None else x.new_empty(0), ln, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = N.lib()
        x, wq, wk, wv, wres, ln, saved = ctx.saved_tensors
        d = ctx.desc
        D = d.D
        use_res = wres.numel() > 0
        scratch = torch.empty(int(lib.satrans_selfatt_scratch_floats(C.byref(d))), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        g = [torch.zeros(D, D, dtype=torch.float32, device=x.device) for _ in range(4)]
        g_ln = torch.zeros(2, D, dtype=torch.float32, device=x.device)
        N.check(lib.satrans_selfatt_bwd(C.byref(d), dy.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), scratch.data_ptr(),
                                        g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr() if use_res else None,
                                        g_ln.data_ptr(), N.stream_handle(x.device)), "satrans_selfatt_bwd")
        return dx, g[0], g[1], g[2], (g[3] if use_res else None), g_ln[0], g_ln[1], None


class SelfAttention_Layer(nn.Module):
    def __init__(self, embedding_size, head_num=2, use_res=True, scaling=True, seed=1024, device='cpu'):
        super().__init__()
        if head_num <= 0:
            raise ValueError('head_num must be a int > 0')
        if embedding_size % head_num != 0:
            raise ValueError('embedding_size is not an integer multiple of head_num!')
        self.att_embedding_size = embedding_size // head_num
        self.head_num, self.use_res, self.scaling, self.seed = head_num, use_res, scaling, seed
        self.W_Query = nn.Parameter(torch.empty(embedding_size, embedding_size))
        self.W_Key = nn.Parameter(torch.empty(embedding_size, embedding_size))
        self.W_Value = nn.Parameter(torch.empty(embedding_size, embedding_size))
        self.W_Out = nn.Parameter(torch.empty(embedding_size, embedding_size))
        self.layer_norm = nn.LayerNorm(embedding_size, eps=1e-6)
        if self.use_res:
            self.W_Res = nn.Parameter(torch.empty(embedding_size, embedding_size))
        for tensor in self.parameters():
            nn.init.normal_(tensor, mean=0.0, std=0.05)
        self.normalized_att_scores = None
        self.capture_attention = False
        self._clock = _DropClock()
        self.to(device)

    def forward(self, inputs):
        if len(inputs.shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(inputs.shape)))
        return _SelfAttFn.apply(inputs, self.W_Query, self.W_Key, self.W_Value, self.W_Res if self.use_res else None,
                                self.layer_norm.weight, self.layer_norm.bias, self)


class _MetaNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, ln_w, ln_b, scenario_ids, mod):
        lib = N.lib()
        N.require_gpu(x, "MetaTransformation")
        x = x.contiguous().float()
        table = table.contiguous().float()
        B, F, D = x.shape
        S = table.shape[0]
        dev = x.device
        order, seg, status = _launch_bucket(scenario_ids.to(torch.int32).contiguous(), B, S, dev)
        st = N.stream_handle(dev)
        d = N.MetaNetDesc()
        d.B, d.F, d.D, d.U, d.S = B, F, D, mod.units[1], S
        d.flags = (N.TRAIN if mod.training else 0) | (0 if mod.use_norm else NO_NORM)
        d.layer, d.drop_p = 0, 0.1
        if mod.training:
            mod._clock.step += 1
        d.seed, d.step = mod._clock.seed, mod._clock.step & 0xFFFFFFFF
        d.tab_stride = table.shape[1]
        ln = torch.cat([ln_w.detach().reshape(-1), ln_b.detach().reshape(-1)]).contiguous() if mod.use_norm else None
        d.x, d.order, d.seg, d.tab = x.data_ptr(), order.data_ptr(), seg.data_ptr(), table.data_ptr()
        d.ln_g = ln.data_ptr() if ln is not None else None
        d.ln_b = ln.data_ptr() + 4 * D if ln is not None else None
        n = int(lib.satrans_metanet_saved_floats(C.byref(d)))
        if n < 0:
            raise N.NativeError(f"MetaTransformation: shape D={D} U={mod.units[1]} is not supported")
        saved = torch.empty(n, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        N.check(lib.satrans_metanet_fwd(C.byref(d), y.data_ptr(), saved.data_ptr(), st), "satrans_metanet_fwd")
        if int(status.item()) != 0:
            raise IndexError("index out of range in self: a scenario id exceeds the scenario table")
        ctx.desc, ctx.mod = d, mod
        ctx.save_for_backward(x, table, ln if ln is not None else x.new_empty(0), saved, order, seg)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = N.lib()
        x, table, ln, saved, order, seg = ctx.saved_tensors
        d = ctx.desc
        scratch = torch.empty(int(lib.satrans_metanet_scratch_floats(C.byref(d))), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        g_tab = torch.zeros_like(table)
        g_ln = torch.zeros(2, d.D, dtype=torch.float32, device=x.device)
        N.check(lib.satrans_metanet_bwd(C.byref(d), dy.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), scratch.data_ptr(),
                                        g_tab.data_ptr(), g_ln.data_ptr() if ln.numel() else None, N.stream_handle(x.device)),
                "satrans_metanet_bwd")
        return dx, g_tab, (g_ln[0] if ln.numel() else None), (g_ln[1] if ln.numel() else None), None, None


class MetaTransformation(nn.Module):
    """`BaseModel.meta_transformation` as a module: scenario ids [B] + embedding block [B,F,D] -> MetaNet(block, weights of the
    sample's scenario).  Parameters in the reference's creation order (models/basemodel.py:137-149): domain_embeddings
    [num_domains+1, D] (torch default N(0,1)), domain_map_dnn = one Linear(D -> P) with weight N(0, 1e-4), meta_net LayerNorm
    (use_norm: the reference's flag 'metanorm')."""

    def __init__(self, embedding_dim, num_domains, meta_dnn_hidden_units=(32, 64, 32), use_norm=False, init_std=0.0001):
        super().__init__()
        units = [int(u) for u in meta_dnn_hidden_units]
        if len(units) != 3 or units[0] != embedding_dim or units[2] != embedding_dim:
            raise NotImplementedError("meta_dnn_hidden_units must be (D, U, D)")
        self.units, self.use_norm = units, use_norm
        self.domain_embeddings = nn.Embedding(num_domains + 1, embedding_dim)
        p = units[0] * units[1] + units[1] * units[2]
        self.domain_map_dnn = nn.Linear(embedding_dim, p)
        nn.init.normal_(self.domain_map_dnn.weight, mean=0, std=init_std)
        self.ffn_layer_norm = nn.LayerNorm(embedding_dim, eps=1e-6) if use_norm else None
        self._clock = _DropClock()

    def forward(self, scenario_ids, fm_input):
        # [S, P] table: S rows through relu + one Linear (a handful of tiny torch ops with autograd; the per-sample work is HIP)
        table = self.domain_map_dnn(torch.relu(self.domain_embeddings.weight))
        w = self.ffn_layer_norm.weight if self.use_norm else None
        b = self.ffn_layer_norm.bias if self.use_norm else None
        return _MetaNetFn.apply(fm_input, table, w, b, scenario_ids.reshape(-1), self)


class _PNormFn(torch.autograd.Function):
    """y = BN_{scenario(i)}(x[i]) for all scenarios at once (csrc/pnorm.hip).  weight, bias [S,C]; running_mean, running_var [S,C]
    or None, updated in place when `batch_stats` (the kernels leave a scenario without rows untouched)."""

    @staticmethod
    def forward(ctx, x, weight, bias, shared_w, shared_b, order, seg, running_mean, running_var, factor, eps, batch_stats):
        lib = N.lib()
        dev = x.device
        x, weight, bias = x.contiguous(), weight.contiguous(), bias.contiguous()
        shared_w, shared_b = shared_w.contiguous(), shared_b.contiguous()
        d = _pnorm_desc(x, weight, bias, shared_w, shared_b, order, seg, running_mean, running_var, factor, eps, batch_stats)
        saved = torch.empty(_native_size(lib.satrans_pnorm_saved_floats, d), dtype=torch.float32, device=dev)
        work = torch.empty(_native_size(lib.satrans_pnorm_workspace_floats, d), dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        N.check(lib.satrans_pnorm_fwd(C.byref(d), y.data_ptr(), saved.data_ptr(), work.data_ptr(), N.stream_handle(dev)),
                "satrans_pnorm_fwd")
        ctx.args = (factor, eps, batch_stats)
        ctx.save_for_backward(x, weight, bias, shared_w, shared_b, order, seg, saved)
        ctx.mark_non_differentiable(saved)
        return y, saved

    @staticmethod
    def backward(ctx, dy, _dsaved):
        lib = N.lib()
        x, weight, bias, shared_w, shared_b, order, seg, saved = ctx.saved_tensors
        d = _pnorm_desc(x, weight, bias, shared_w, shared_b, order, seg, None, None, *ctx.args)
        work = torch.empty(_native_size(lib.satrans_pnorm_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx, g_w, g_b = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(bias)
        g_sw, g_sb = torch.empty_like(shared_w), torch.empty_like(shared_b)
        N.check(lib.satrans_pnorm_bwd(C.byref(d), dy.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                      g_w.data_ptr(), g_b.data_ptr(), g_sw.data_ptr(), g_sb.data_ptr(), N.stream_handle(x.device)),
                "satrans_pnorm_bwd")
        return dx, g_w, g_b, g_sw, g_sb, None, None, None, None, None, None, None


def _pnorm_desc(x, weight, bias, shared_w, shared_b, order, seg, running_mean, running_var, factor, eps, batch_stats):
    d = N.PNormDesc()
    d.B, d.C, d.S = x.shape[0], x.shape[1], weight.shape[0]
    d.flags, d.eps, d.factor = (N.TRAIN if batch_stats else 0), eps, factor
    d.x, d.order, d.seg = x.data_ptr(), order.data_ptr(), seg.data_ptr()
    d.weight, d.bias, d.shared_w, d.shared_b = weight.data_ptr(), bias.data_ptr(), shared_w.data_ptr(), shared_b.data_ptr()
    d.running_mean = running_mean.data_ptr() if running_mean is not None else None
    d.running_var = running_var.data_ptr() if running_var is not None else None
    return d


def _native_size(fn, d):
    n = int(fn(C.byref(d)))
    if n < 0:
        N.check(n, fn.__name__)
    return n


def _pnorm_check_input(x, shared_weight, shared_bias, num_features, what):
    if x.dim() == 3:
        raise NotImplementedError(f"{what}: 3-D input is not built; pass the 2-D form [n, C] (the reference's only caller does)")
    if x.dim() != 2:
        raise ValueError("expected 2D or 3D input (got {}D input)".format(x.dim()))
    N.require_gpu(x, what)
    if x.dtype != torch.float32 or shared_weight.dtype != torch.float32 or shared_bias.dtype != torch.float32:
        raise TypeError(f"{what}: rows, parameters and gradients are float32")
    if x.shape[1] != num_features or shared_weight.numel() != num_features or shared_bias.numel() != num_features:
        raise ValueError(f"{what}: expected {num_features} channels, got input {tuple(x.shape)}, shared weight "
                         f"{tuple(shared_weight.shape)}, shared bias {tuple(shared_bias.shape)}")


def _pnorm_run(bns, x, order, seg, counts, shared_weight, shared_bias, training):
    """The reference's MDR_BatchNorm.forward for every module of `bns` at once (module s owns the rows of scenario s; `counts` are
    the host-side row counts).  Every check runs before the first buffer is written.  -> y, [2,S,C] = the mean and
    1 / sqrt(var + eps) the forward normalised with (the modules keep it as `last_stats`)."""
    first = bns[0]
    tracked = first.track_running_stats
    batch_stats = training or not tracked                 # reference: training, or evaluation without buffers
    if batch_stats and 1 in counts:                       # torch.nn.functional._verify_batch_size
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(
            torch.Size([1, x.shape[1]])))
    factor = 0.0 if first.momentum is None else float(first.momentum)
    update = training and tracked
    if update and first.momentum is None:                 # cumulative average: 1 / num_batches_tracked, after its increment
        seen = set(torch.stack([m.num_batches_tracked for m in bns]).tolist())
        if len(seen) != 1:
            raise NotImplementedError("momentum=None with num_batches_tracked differing between the scenarios' modules")
        factor = 1.0 / float(seen.pop() + 1)
    if update:
        torch._foreach_add_([m.num_batches_tracked for m in bns], 1)
    running_mean = running_var = None
    if tracked:
        running_mean = torch.stack([m.running_mean for m in bns])
        running_var = torch.stack([m.running_var for m in bns])
    weight, bias = torch.stack([m.weight for m in bns]), torch.stack([m.bias for m in bns])
    y, saved = _PNormFn.apply(x, weight, bias, shared_weight.reshape(-1), shared_bias.reshape(-1), order, seg, running_mean,
                          running_var, factor, float(first.eps), batch_stats)
    if update:
        with torch.no_grad():
            torch._foreach_copy_([m.running_mean for m in bns] + [m.running_var for m in bns],
                                 list(running_mean.unbind(0)) + list(running_var.unbind(0)))
    return y, saved.view(2, len(bns), -1)


def _launch_bucket(sid_in, B, S, dev):
    """satrans_bucket_scenarios on B int32 ids -> order [B], seg [S+1], status [1] (non-zero: an id outside [0, S)); no read-back."""
    lib = N.lib()
    i32 = dict(dtype=torch.int32, device=dev)
    sid, order, seg = torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(S + 1, **i32)
    status = torch.zeros(1, **i32)
    bucket = torch.empty(int(lib.satrans_bucket_workspace_bytes(B, S)), dtype=torch.uint8, device=dev)
    N.check(lib.satrans_bucket_scenarios(sid_in.data_ptr(), N.ID_I32, 1, 0, B, S, sid.data_ptr(), order.data_ptr(), seg.data_ptr(),
                                         status.data_ptr(), bucket.data_ptr(), bucket.numel(), N.stream_handle(dev)),
            "satrans_bucket_scenarios")
    return order, seg, status


def _bucket_rows(x, domain_ids, S, domain_id_offset, what):
    """Bucket the rows of x by scenario id - offset (satrans_bucket_scenarios) -> order [B], seg [S+1] on the device and the
    host-side row counts.  One device-to-host read (the S + 1 segment bounds and the status word); an id outside
    [offset, offset + S) raises IndexError."""
    B, dev = x.shape[0], x.device
    if B == 0 or domain_ids.numel() != B:
        raise ValueError(f"{what}: {B} rows with {domain_ids.numel()} scenario ids")
    sid_in = (domain_ids.reshape(-1).to(device=dev, dtype=torch.int64) - int(domain_id_offset)).to(torch.int32).contiguous()
    order, seg, status = _launch_bucket(sid_in, B, S, dev)
    host = torch.cat([seg, status]).tolist()
    if host[-1] != 0:
        raise IndexError(f"{what}: a scenario id lies outside [{domain_id_offset}, {domain_id_offset + S})")
    return order, seg, [host[s + 1] - host[s] for s in range(S)]


class MDR_BatchNorm(_NormBase):
    """One scenario's batch-norm whose scale and shift are multiplied / added onto a shared pair:
    F.batch_norm(input, running_mean, running_var, weight * shared_weight, bias + shared_bias, ...).  Parameters, buffers,
    state_dict keys, the momentum=None rule (cumulative average, factor 1 / num_batches_tracked) and the rule for when batch
    statistics are used are the reference's.  affine=False is refused at construction (the reference's forward would compute
    None * tensor); 3-D input is not built.  Internally the one-scenario case of PartitionedNorm's launches."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None):
        if not affine:
            raise ValueError("MDR_BatchNorm needs affine=True: its forward multiplies weight by the shared weight")
        if dtype not in (None, torch.float32):
            raise TypeError("MDR_BatchNorm: parameters are float32")
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device=device, dtype=dtype)
        self.last_stats = None

    def _check_input_dim(self, input):
        if input.dim() != 2 and input.dim() != 3:
            raise ValueError("expected 2D or 3D input (got {}D input)".format(input.dim()))

    def forward(self, input, shared_weight, shared_bias):
        _pnorm_check_input(input, shared_weight, shared_bias, self.num_features, "MDR_BatchNorm")
        n = input.shape[0]
        if n == 0:      # torch: an empty input passes through, the running statistics stay, the batch is counted
            if self.training and self.track_running_stats:
                self.num_batches_tracked.add_(1)
            return input * (self.weight * shared_weight) + (self.bias + shared_bias)
        order = torch.arange(n, dtype=torch.int32, device=input.device)
        seg = torch.tensor([0, n], dtype=torch.int32, device=input.device)
        y, self.last_stats = _pnorm_run([self], input, order, seg, [n], shared_weight, shared_bias, self.training)
        return y


class PartitionedNorm(nn.Module):
    """STAR's partitioned normalisation: `bns = ModuleList(MDR_BatchNorm(num_features) for each scenario)` (state_dict keys
    `bns.{i}.*`, as in the reference's Star_Net) applied to a mixed batch in one pass.  Replaces the loop of models/star.py:147-154

        for i in range(num_domains):
            rows = x[domain_ids == i + domain_id_offset]
            out[domain_ids == i + domain_id_offset] = bns[i](rows, shared_weight, shared_bias)

    by: bucket the ids (satrans_bucket_scenarios), one forward over all scenarios, every module's num_batches_tracked
    incremented as the loop does (a scenario without rows keeps its running statistics, as torch does for an empty input).

    Differences from the loop.  (1) A scenario with exactly ONE row in training mode raises torch's ValueError("Expected more
    than 1 value per channel when training, ...") BEFORE any buffer is written; in the loop the scenarios in front of the
    offending one would already have updated theirs.  (2) An id outside [offset, offset + num_domains) raises IndexError; the
    loop silently leaves such rows out.  One device-to-host read per forward (the S + 1 segment bounds) serves both checks."""

    def __init__(self, num_features, num_domains, eps=1e-5, momentum=0.1):
        super().__init__()
        if num_domains < 1:
            raise ValueError("num_domains must be >= 1")
        self.num_features, self.num_domains = num_features, num_domains
        self.bns = nn.ModuleList([MDR_BatchNorm(num_features, eps=eps, momentum=momentum) for _ in range(num_domains)])
        self.last_stats = None

    def forward(self, x, domain_ids, shared_weight, shared_bias, domain_id_offset=0):
        _pnorm_check_input(x, shared_weight, shared_bias, self.num_features, "PartitionedNorm")
        order, seg, counts = _bucket_rows(x, domain_ids, self.num_domains, domain_id_offset, "PartitionedNorm")
        y, self.last_stats = _pnorm_run(list(self.bns), x, order, seg, counts, shared_weight, shared_bias, self.training)
        return y


class _StarFn(torch.autograd.Function):
    """logit [B,1] of the towers for all scenarios at once (csrc/star.hip).  `tensors` = L stacked per-scenario weights
    [S, n_l, n_{l-1}], L stacked biases [S, n_l], L shared weights, L shared biases."""

    @staticmethod
    def forward(ctx, x, order, seg, L, *tensors):
        lib = N.lib()
        dev = x.device
        x = x.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        d = _star_desc(x, order, seg, L, tensors)
        saved = torch.empty(_native_size(lib.satrans_star_saved_floats, d), dtype=torch.float32, device=dev)
        logit = torch.empty(x.shape[0], 1, dtype=torch.float32, device=dev)
        N.check(lib.satrans_star_fwd(C.byref(d), logit.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_star_fwd")
        ctx.L = L
        ctx.save_for_backward(x, order, seg, saved, *tensors)
        ctx.mark_non_differentiable(saved)
        return logit, saved

    @staticmethod
    def backward(ctx, dlogit, _dsaved):
        lib = N.lib()
        x, order, seg, saved, *tensors = ctx.saved_tensors
        L = ctx.L
        d = _star_desc(x, order, seg, L, tensors)
        work = torch.empty(_native_size(lib.satrans_star_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(t) for t in tensors]
        groups = [(C.c_void_p * L)(*[g.data_ptr() for g in grads[k * L:(k + 1) * L]]) for k in range(4)]
        N.check(lib.satrans_star_bwd(C.byref(d), dlogit.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                     groups[0], groups[1], groups[2], groups[3], N.stream_handle(x.device)), "satrans_star_bwd")
        return (dx, None, None, None, *grads)


def _star_desc(x, order, seg, L, tensors):
    d = N.StarDesc()
    d.B, d.C, d.S, d.L = x.shape[0], x.shape[1], tensors[0].shape[0], L
    d.x, d.order, d.seg = x.data_ptr(), order.data_ptr(), seg.data_ptr()
    for l in range(L):
        d.width[l] = tensors[l].shape[1]
        d.w_dom[l], d.b_dom[l] = tensors[l].data_ptr(), tensors[L + l].data_ptr()
        d.w_sh[l], d.b_sh[l] = tensors[2 * L + l].data_ptr(), tensors[3 * L + l].data_ptr()
    return d


class _TowerDNN(nn.Module):
    """The Linear layers of the reference's DNN (state_dict keys `linears.{l}.{weight,bias}`); relu, no dropout, no batch-norm.
    A holder of parameters: the towers' arithmetic runs in csrc/star.hip."""

    def __init__(self, inputs_dim, hidden_units, init_std):
        super().__init__()
        units = [inputs_dim] + list(hidden_units)
        self.linears = nn.ModuleList([nn.Linear(units[i], units[i + 1]) for i in range(len(units) - 1)])
        for lin in self.linears:
            nn.init.normal_(lin.weight, mean=0, std=init_std)


class StarTowers(nn.Module):
    """STAR's star-topology FC towers over a mixed batch: scenario s applies, layer by layer,

        relu(F.linear(h, domain_dnns[s].linears[l].weight * shared_dnn.linears[l].weight,
                         domain_dnns[s].linears[l].bias + shared_dnn.linears[l].bias))

    and at the end F.linear(h, domain_dnn_linears[s].weight * shared_dnn_linear.weight, the two biases summed) to the rows
    whose id is s + domain_id_offset - the loop of models/star.py:147-170 without its normalisation.  Parameter names, shapes
    and initialisation are the reference Star_Net's (weights of the towers N(0, init_std); biases and the final nn.Linears
    torch's default), so the tower entries of a reference checkpoint load with load_state_dict.

    forward(x [B, inputs_dim] fp32, domain_ids [B], domain_id_offset=0) -> logit [B,1]; the caller applies the sigmoid.
    Per call: the per-scenario parameters are stacked (torch.stack; autograd splits the gradients back), the ids bucketed
    (one device-to-host read), and one autograd.Function runs satrans_star_fwd / satrans_star_bwd.  `last_hidden` holds the
    hidden rows of the last forward, [B, n_l] per hidden layer.

    Differences from the loop.  An id outside [offset, offset + num_domains) raises IndexError; the loop silently leaves such
    rows at logit 0.  Not built (main.py passes none of them): an activation other than relu, dropout, batch-norm inside the
    towers - NotImplementedError at construction.  1 to 4 hidden layers of any positive width."""

    def __init__(self, inputs_dim, hidden_units=(256, 128), num_domains=1, init_std=0.0001, activation='relu', dropout_rate=0,
                 use_bn=False):
        super().__init__()
        self._build_towers(inputs_dim, hidden_units, num_domains, init_std, activation, dropout_rate, use_bn)

    def _build_towers(self, inputs_dim, hidden_units, num_domains, init_std, activation, dropout_rate, use_bn):
        if activation != 'relu':
            raise NotImplementedError(f"StarTowers: activation {activation!r} is not built (relu only)")
        if dropout_rate != 0:
            raise NotImplementedError("StarTowers: dropout inside the towers is not built (dropout_rate must be 0)")
        if use_bn:
            raise NotImplementedError("StarTowers: batch-norm inside the towers is not built (use_bn must be False)")
        hidden_units = [int(u) for u in hidden_units]
        if not 1 <= len(hidden_units) <= N.STAR_MAX_LAYERS - 1:
            raise NotImplementedError(f"StarTowers: 1 to {N.STAR_MAX_LAYERS - 1} hidden layers, got {len(hidden_units)}")
        if inputs_dim < 1 or min(hidden_units) < 1 or num_domains < 1:
            raise ValueError("StarTowers: inputs_dim, hidden_units and num_domains must be positive")
        self.inputs_dim, self.hidden_units, self.num_domains = int(inputs_dim), tuple(hidden_units), int(num_domains)
        self.domain_dnns = nn.ModuleList([_TowerDNN(inputs_dim, hidden_units, init_std) for _ in range(num_domains)])
        self.domain_dnn_linears = nn.ModuleList([nn.Linear(hidden_units[-1], 1) for _ in range(num_domains)])
        self.shared_dnn = _TowerDNN(inputs_dim, hidden_units, init_std)
        self.shared_dnn_linear = nn.Linear(hidden_units[-1], 1)
        self.last_hidden = None

    def _check_input(self, x, what):
        if x.dim() != 2 or x.shape[1] != self.inputs_dim:
            raise ValueError(f"{what}: expected input [B, {self.inputs_dim}], got {tuple(x.shape)}")
        N.require_gpu(x, what)
        if x.dtype != torch.float32 or self.shared_dnn_linear.weight.dtype != torch.float32:
            raise TypeError(f"{what}: rows, parameters and gradients are float32")

    def _run_towers(self, x, order, seg):
        S, H = self.num_domains, len(self.hidden_units)
        doms = [[self.domain_dnns[s].linears[l] for s in range(S)] for l in range(H)] + [list(self.domain_dnn_linears)]
        shared = list(self.shared_dnn.linears) + [self.shared_dnn_linear]
        tensors = ([torch.stack([m.weight for m in layer]) for layer in doms] + [torch.stack([m.bias for m in layer]) for layer in doms]
                   + [m.weight for m in shared] + [m.bias for m in shared])
        logit, saved = _StarFn.apply(x, order, seg, H + 1, *tensors)
        B, at, self.last_hidden = x.shape[0], 0, []
        for n in self.hidden_units:
            self.last_hidden.append(saved[at:at + B * n].view(B, n))
            at += B * n
        return logit

    def forward(self, x, domain_ids, domain_id_offset=0):
        self._check_input(x, "StarTowers")
        order, seg, _ = _bucket_rows(x, domain_ids, self.num_domains, domain_id_offset, "StarTowers")
        return self._run_towers(x, order, seg)


class StarHead(StarTowers):
    """The scenario-dependent half of the reference's Star_Net.forward (models/star.py:144-173) as one module: the partitioned
    normalisation (when use_domain_bn), then the star-topology towers, on ONE bucketing of the batch.  Owns, under the
    reference's top-level names, shared_bn_weight, shared_bn_bias, bns.{s}.* (MDR_BatchNorm; only with use_domain_bn) and the
    four tower groups of StarTowers, in the reference's creation order.

    forward(dnn_input [B, inputs_dim], domain_ids [B], domain_id_offset=0) -> logit [B,1]; the caller applies the sigmoid.
    PartitionedNorm's differences from the loop hold here too: a scenario with exactly one row in training mode raises torch's
    ValueError before any buffer is written, an id out of range raises IndexError.  Without use_domain_bn the shared
    normalisation parameters exist and stay unused, as in the reference."""

    def __init__(self, inputs_dim, hidden_units=(256, 128), num_domains=1, use_domain_bn=True, init_std=0.0001, activation='relu',
                 dropout_rate=0, use_bn=False, eps=1e-5, momentum=0.1):
        nn.Module.__init__(self)
        self.use_domain_bn = bool(use_domain_bn)
        self.shared_bn_weight = nn.Parameter(torch.ones(inputs_dim))
        self.shared_bn_bias = nn.Parameter(torch.zeros(inputs_dim))
        if self.use_domain_bn:
            self.bns = nn.ModuleList([MDR_BatchNorm(inputs_dim, eps=eps, momentum=momentum) for _ in range(num_domains)])
        self._build_towers(inputs_dim, hidden_units, num_domains, init_std, activation, dropout_rate, use_bn)
        self.last_stats = None

    def forward(self, dnn_input, domain_ids, domain_id_offset=0):
        self._check_input(dnn_input, "StarHead")
        if self.use_domain_bn:
            _pnorm_check_input(dnn_input, self.shared_bn_weight, self.shared_bn_bias, self.inputs_dim, "StarHead")
        order, seg, counts = _bucket_rows(dnn_input, domain_ids, self.num_domains, domain_id_offset, "StarHead")
        h = dnn_input
        if self.use_domain_bn:
            h, self.last_stats = _pnorm_run(list(self.bns), h, order, seg, counts, self.shared_bn_weight, self.shared_bn_bias,
                                            self.training)
        return self._run_towers(h, order, seg)


def _mmoe_fill(d, x, order, seg, cfg, tensors, out=None):
    """Fill a satrans_mmoe_desc (out is None) or the satrans_mmoe_grads `out` from `tensors`, which hold, in this order:
    expert weights, expert biases, gate weights, gate biases, the gate's final weight, tower weights, tower biases, the tower's
    final weight, the out biases (stacked over experts or tasks)."""
    nx, ng, nt = cfg
    it = iter(tensors)
    tgt = d if out is None else out
    for name, n in (("expert_w", nx), ("expert_b", nx), ("gate_w", ng), ("gate_b", ng)):
        for l in range(n):
            getattr(tgt, name)[l] = next(it).data_ptr()
    tgt.gate_final_w = next(it).data_ptr()
    for name, n in (("tower_w", nt), ("tower_b", nt)):
        for l in range(n):
            getattr(tgt, name)[l] = next(it).data_ptr()
    tgt.tower_final_w = next(it).data_ptr()
    tgt.out_bias = next(it).data_ptr()
    if out is None:
        d.B, d.C, d.T, d.E = x.shape[0], x.shape[1], tensors[-1].shape[0], tensors[0].shape[0]
        d.n_expert, d.n_gate, d.n_tower = nx, ng, nt
        d.x, d.order, d.seg = x.data_ptr(), order.data_ptr(), seg.data_ptr()
        for l in range(nx):
            d.expert_width[l] = tensors[l].shape[1]
        for l in range(ng):
            d.gate_width[l] = tensors[2 * nx + l].shape[1]
        for l in range(nt):
            d.tower_width[l] = tensors[2 * nx + 2 * ng + 1 + l].shape[1]
    return tgt


class _MMoEFn(torch.autograd.Function):
    """logit [B,1] of the scenario-routed MMoE head (csrc/mmoe.hip); `tensors` as _mmoe_fill lists them."""

    @staticmethod
    def forward(ctx, x, order, seg, cfg, *tensors):
        lib = N.lib()
        dev = x.device
        x = x.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        d = _mmoe_fill(N.MMoEDesc(), x, order, seg, cfg, tensors)
        saved = torch.empty(_native_size(lib.satrans_mmoe_saved_floats, d), dtype=torch.float32, device=dev)
        logit = torch.empty(x.shape[0], 1, dtype=torch.float32, device=dev)
        N.check(lib.satrans_mmoe_fwd(C.byref(d), logit.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_mmoe_fwd")
        ctx.cfg = cfg
        ctx.save_for_backward(x, order, seg, saved, *tensors)
        ctx.mark_non_differentiable(saved)
        return logit, saved

    @staticmethod
    def backward(ctx, dlogit, _dsaved):
        lib = N.lib()
        x, order, seg, saved, *tensors = ctx.saved_tensors
        d = _mmoe_fill(N.MMoEDesc(), x, order, seg, ctx.cfg, tensors)
        work = torch.empty(_native_size(lib.satrans_mmoe_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(t) for t in tensors]
        g = _mmoe_fill(d, x, order, seg, ctx.cfg, grads, out=N.MMoEGrads())
        N.check(lib.satrans_mmoe_bwd(C.byref(d), dlogit.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                     C.byref(g), N.stream_handle(x.device)), "satrans_mmoe_bwd")
        return (dx, None, None, None, *grads)


class _OutBias(nn.Module):
    """The parameter of deepctr's PredictionLayer (state_dict key `bias`, shape [1], zeros); MMoEHead adds it to the logit."""

    def __init__(self):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros((1,)))


class MMoEHead(nn.Module):
    """The expert / gate / tower half of the reference's MMOE.forward (models/mmoe.py:142-171) over a mixed batch, for the
    reference's one-task-per-scenario use (T = tasks = scenarios): the loss of mtl_basemodel.py:268-269 and predict (:376-378)
    read, of a row's T outputs, only the column of the row's own scenario.  So the E experts run over all rows, and a row
    whose id is t + domain_id_offset goes through task t's gate DNN and gate_dnn_final_layer, the softmax mixture of the
    experts' outputs, task t's tower DNN and tower_dnn_final_layer, and out[t].bias - nothing of the other tasks.

    Parameter names, shapes, state_dict order and initialisation are the reference MMOE's (DNN weights N(0, init_std), their
    biases and the bias-free final nn.Linears torch's default, out.{t}.bias zeros): expert_dnn.{e}.linears.{l}.*,
    gate_dnn.{t}.linears.{l}.* (only with gate hidden units), gate_dnn_final_layer.{t}.weight, tower_dnn.{t}.linears.{l}.*
    (only with tower hidden units), tower_dnn_final_layer.{t}.weight, out.{t}.bias - those entries of a reference checkpoint
    load with load_state_dict.

    forward(dnn_input [B, inputs_dim] fp32, domain_ids [B], domain_id_offset=0) -> logit [B,1]; the caller applies the
    sigmoid.  Per call: the ids are bucketed once (one device-to-host read), the per-task and per-expert parameters stacked
    (torch.stack; autograd splits the gradients back), and one autograd.Function runs satrans_mmoe_fwd / satrans_mmoe_bwd.
    `last_gates` [B, E] and `last_mixture` [B, last expert width] are views of the last forward's saved buffer.

    Differences from the reference.  (1) The module returns each row's OWN task logit, [B,1], not the [B,T] matrix of all
    tasks: the other T - 1 columns are never computed.  (2) l2_reg_dnn is not applied (main.py leaves it 0).  (3) An id
    outside [offset, offset + num_tasks) raises IndexError; the reference's loss silently leaves such rows out.
    Not built - NotImplementedError at construction: an activation other than relu, dropout, batch-norm inside the DNNs,
    more than 8 experts, more than 3 hidden layers in a DNN, no expert layer."""

    def __init__(self, inputs_dim, num_tasks, num_experts=3, expert_dnn_hidden_units=(256, 128), gate_dnn_hidden_units=(64,),
                 tower_dnn_hidden_units=(64,), init_std=0.0001, dnn_activation='relu', dnn_dropout=0, dnn_use_bn=False):
        super().__init__()
        if dnn_activation != 'relu':
            raise NotImplementedError(f"MMoEHead: activation {dnn_activation!r} is not built (relu only)")
        if dnn_dropout != 0:
            raise NotImplementedError("MMoEHead: dropout inside the DNNs is not built (dnn_dropout must be 0)")
        if dnn_use_bn:
            raise NotImplementedError("MMoEHead: batch-norm inside the DNNs is not built (dnn_use_bn must be False)")
        if num_tasks <= 1:
            raise ValueError("num_tasks must be greater than 1")
        if num_experts <= 1:
            raise ValueError("num_experts must be greater than 1")
        if num_experts > N.MMOE_MAX_EXPERTS:
            raise NotImplementedError(f"MMoEHead: 2 to {N.MMOE_MAX_EXPERTS} experts, got {num_experts}")
        ex, ga, to = ([int(u) for u in units] for units in (expert_dnn_hidden_units, gate_dnn_hidden_units, tower_dnn_hidden_units))
        if not 1 <= len(ex) <= N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"MMoEHead: 1 to {N.MMOE_MAX_HIDDEN} expert hidden layers, got {len(ex)}")
        if len(ga) > N.MMOE_MAX_HIDDEN or len(to) > N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"MMoEHead: 0 to {N.MMOE_MAX_HIDDEN} gate and tower hidden layers, got {len(ga)} and {len(to)}")
        if inputs_dim < 1 or min(ex + ga + to) < 1:
            raise ValueError("MMoEHead: inputs_dim and the hidden units must be positive")
        self.inputs_dim, self.num_tasks, self.num_experts = int(inputs_dim), int(num_tasks), int(num_experts)
        self.expert_dnn_hidden_units, self.gate_dnn_hidden_units, self.tower_dnn_hidden_units = tuple(ex), tuple(ga), tuple(to)
        T, E = self.num_tasks, self.num_experts
        # (first: in the reference's state_dict `out.*` precedes MMOE's own modules, because its BaseModel registers that name)
        self.out = nn.ModuleList([_OutBias() for _ in range(T)])
        self.expert_dnn = nn.ModuleList([_TowerDNN(inputs_dim, ex, init_std) for _ in range(E)])
        if ga:
            self.gate_dnn = nn.ModuleList([_TowerDNN(inputs_dim, ga, init_std) for _ in range(T)])
        self.gate_dnn_final_layer = nn.ModuleList([nn.Linear(ga[-1] if ga else inputs_dim, E, bias=False) for _ in range(T)])
        if to:
            self.tower_dnn = nn.ModuleList([_TowerDNN(ex[-1], to, init_std) for _ in range(T)])
        self.tower_dnn_final_layer = nn.ModuleList([nn.Linear(to[-1] if to else ex[-1], 1, bias=False) for _ in range(T)])
        self.last_gates = self.last_mixture = None

    def forward(self, dnn_input, domain_ids, domain_id_offset=0):
        x = dnn_input
        if x.dim() != 2 or x.shape[1] != self.inputs_dim:
            raise ValueError(f"MMoEHead: expected input [B, {self.inputs_dim}], got {tuple(x.shape)}")
        N.require_gpu(x, "MMoEHead")
        if x.dtype != torch.float32 or self.out[0].bias.dtype != torch.float32:
            raise TypeError("MMoEHead: rows, parameters and gradients are float32")
        order, seg, _ = _bucket_rows(x, domain_ids, self.num_tasks, domain_id_offset, "MMoEHead")
        nx, ng, nt = len(self.expert_dnn_hidden_units), len(self.gate_dnn_hidden_units), len(self.tower_dnn_hidden_units)

        def stacked(dnns, n):
            layers = [[m.linears[l] for m in dnns] for l in range(n)]
            return ([torch.stack([m.weight for m in layer]) for layer in layers] +
                    [torch.stack([m.bias for m in layer]) for layer in layers])

        tensors = (stacked(self.expert_dnn, nx) + (stacked(self.gate_dnn, ng) if ng else []) +
                   [torch.stack([m.weight for m in self.gate_dnn_final_layer])] + (stacked(self.tower_dnn, nt) if nt else []) +
                   [torch.stack([m.weight for m in self.tower_dnn_final_layer]), torch.cat([m.bias for m in self.out])])
        logit, saved = _MMoEFn.apply(x, order, seg, (nx, ng, nt), *tensors)
        B, E, n = x.shape[0], self.num_experts, self.expert_dnn_hidden_units[-1]
        self.last_gates = saved[:B * E].view(B, E)
        self.last_mixture = saved[B * E:B * (E + n)].view(B, n)
        return logit


def _ple_counts(cfg):
    """How many tensors each pointer of N.PLE_POINTERS takes from the list (0: not passed), for cfg = (levels, ns, nsh, nx, ng, nt)."""
    levels, _, _, nx, ng, nt = cfg
    per = {"e0": nx, "g0": ng, "sg0": ng, "spec": nx, "shared": nx, "gate": ng, "tower": nt}
    out = []
    for name, per_layer in N.PLE_POINTERS:
        lower = name.split("_")[0] in ("e0", "g0", "sg0")
        out.append((name, per_layer, 0 if lower and levels == 1 else (per[name.split("_")[0]] if per_layer else 1)))
    return out


def _ple_fill(tgt, cfg, tensors):
    """Set the parameter pointers of a satrans_ple_desc or satrans_ple_grads from `tensors`, which follow N.PLE_POINTERS (a
    per-layer pointer takes one tensor per hidden layer; the level-0 pointers take none with one level)."""
    it = iter(tensors)
    for name, per_layer, n in _ple_counts(cfg):
        for l in range(n):
            if per_layer:
                getattr(tgt, name)[l] = next(it).data_ptr()
            else:
                setattr(tgt, name, next(it).data_ptr())
    return tgt


def _ple_desc(x, order, seg, task, cfg, widths, T, tensors):
    d = _ple_fill(N.PLEDesc(), cfg, tensors)
    d.B, d.C, d.T = x.shape[0], x.shape[1], T
    d.levels, d.ns, d.nsh, d.n_expert, d.n_gate, d.n_tower = cfg
    for arr, units in zip((d.expert_width, d.gate_width, d.tower_width), widths):
        for l, n in enumerate(units):
            arr[l] = n
    d.x, d.order, d.seg, d.task = x.data_ptr(), order.data_ptr(), seg.data_ptr(), task.data_ptr()
    return d


class _PLEFn(torch.autograd.Function):
    """logit [B,1] of the scenario-routed PLE head (csrc/ple.hip); `tensors` as _ple_fill lists them."""

    @staticmethod
    def forward(ctx, x, order, seg, task, cfg, widths, T, *tensors):
        lib = N.lib()
        dev = x.device
        x = x.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        d = _ple_desc(x, order, seg, task, cfg, widths, T, tensors)
        saved = torch.empty(_native_size(lib.satrans_ple_saved_floats, d), dtype=torch.float32, device=dev)
        logit = torch.empty(x.shape[0], 1, dtype=torch.float32, device=dev)
        N.check(lib.satrans_ple_fwd(C.byref(d), logit.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_ple_fwd")
        ctx.cfg = (cfg, widths, T)
        ctx.save_for_backward(x, order, seg, task, saved, *tensors)
        ctx.mark_non_differentiable(saved)
        return logit, saved

    @staticmethod
    def backward(ctx, dlogit, _dsaved):
        lib = N.lib()
        x, order, seg, task, saved, *tensors = ctx.saved_tensors
        cfg, widths, T = ctx.cfg
        d = _ple_desc(x, order, seg, task, cfg, widths, T, tensors)
        work = torch.empty(_native_size(lib.satrans_ple_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(t) for t in tensors]
        g = _ple_fill(N.PLEGrads(), cfg, grads)
        N.check(lib.satrans_ple_bwd(C.byref(d), dlogit.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                    C.byref(g), N.stream_handle(x.device)), "satrans_ple_bwd")
        return (dx, None, None, None, None, None, None, *grads)


class PLEHead(nn.Module):
    """The expert / gate / tower half of the reference's PLE.forward (models/ple.py:161-248) over a mixed batch, for the
    reference's one-task-per-scenario use (T = tasks = scenarios): the loss of mtl_basemodel.py:268-269 and predict read, of a
    row's T outputs, only the column of the row's own scenario.  With two CGC levels a row whose id is t + domain_id_offset
    therefore goes through: every level-0 expert (all T * specific + shared of them: the shared mixture needs each) and the
    level-0 shared gate, as every row does; task t's level-0 gate and mixture over its own and the shared experts; on the last
    level task t's specific experts, gate and mixture, the shared experts over the shared mixture, task t's tower and
    out[t].bias - and nothing of the other tasks.  With one level only the last-level part exists, over dnn_input.

    Parameter names, shapes, state_dict order and initialisation are the reference PLE's (DNN weights N(0, init_std), their
    biases and the bias-free final nn.Linears torch's default, out.{t}.bias zeros): out.{t}.bias,
    specific_experts.{level}.{task}.{j}.linears.{l}.*, shared_experts.{level}.0.{k}.linears.{l}.*,
    specific_gate_dnn.{level}.{task}.0.linears.{l}.* and shared_gate_dnn.{level}.linears.{l}.* (only with gate hidden units),
    specific_gate_dnn_final_layer.{level}.{task}.weight, shared_gate_dnn_final_layer.{level}.weight, tower_dnn.{t}.linears.{l}.*
    (only with tower hidden units), tower_dnn_final_layer.{t}.weight - those entries of a reference checkpoint load with
    load_state_dict.  Two kinds of parameter exist only for that and are never handed to the kernels; their .grad stays None,
    exactly as in the reference: the LAST level's shared gate (its mixture feeds nothing), and shared_experts.{level}.0.{k} for
    k >= shared_expert_num (the reference builds specific_expert_num shared experts per level and uses shared_expert_num).

    forward(dnn_input [B, inputs_dim] fp32, domain_ids [B], domain_id_offset=0) -> logit [B,1]; the caller applies the
    sigmoid.  Per call: the ids are bucketed once (one device-to-host read), the row-to-task array is formed, the parameters
    stacked (torch.stack; autograd splits the gradients back), and one autograd.Function runs satrans_ple_fwd /
    satrans_ple_bwd.  `last_gates` [B, specific + shared] and `last_mixture` [B, last expert width] are views of the last
    forward's saved buffer, taken from the LAST level.  A task without rows gets zeros in its routed gradients.

    Differences from the reference.  (1) The module returns each row's OWN task logit, [B,1], not the [B,T] matrix of all
    tasks: the other T - 1 columns are never computed.  (2) l2_reg_dnn is not applied (main.py leaves it 0).  (3) One or two
    levels: with three or more, the gates of levels below the last but one receive gradient from every row through the shared
    mixture of the level above, so nothing is left to route there - a different kernel plan, not built.  (4) An id outside
    [offset, offset + num_tasks) raises IndexError; the reference's loss silently leaves such rows out.
    (5) shared_expert_num > specific_expert_num raises ValueError at construction; the reference raises IndexError in its
    forward.  Not built - NotImplementedError at construction: num_levels outside {1, 2}, more than 8 experts under a task's
    gate (specific + shared), more than 64 under the level-0 shared gate (num_tasks * specific + shared), more than 3 hidden
    layers in a DNN, no expert layer, an activation other than relu, dropout, batch-norm inside the DNNs."""

    def __init__(self, inputs_dim, num_tasks, shared_expert_num=1, specific_expert_num=1, num_levels=2,
                 expert_dnn_hidden_units=(256, 128), gate_dnn_hidden_units=(64,), tower_dnn_hidden_units=(64,), init_std=0.0001,
                 dnn_activation='relu', dnn_dropout=0, dnn_use_bn=False):
        super().__init__()
        if dnn_activation != 'relu':
            raise NotImplementedError(f"PLEHead: activation {dnn_activation!r} is not built (relu only)")
        if dnn_dropout != 0:
            raise NotImplementedError("PLEHead: dropout inside the DNNs is not built (dnn_dropout must be 0)")
        if dnn_use_bn:
            raise NotImplementedError("PLEHead: batch-norm inside the DNNs is not built (dnn_use_bn must be False)")
        if num_tasks <= 1:
            raise ValueError("num_tasks must be greater than 1")
        T, ns, nsh, levels = int(num_tasks), int(specific_expert_num), int(shared_expert_num), int(num_levels)
        if nsh < 1 or ns < 1:
            raise ValueError(f"PLEHead: shared_expert_num and specific_expert_num must be at least 1, got {nsh} and {ns}")
        if nsh > ns:
            raise ValueError(f"PLEHead: shared_expert_num {nsh} > specific_expert_num {ns}: the reference builds specific_expert_num "
                             "shared experts per level and raises IndexError in its forward")
        if levels not in (1, 2):
            raise NotImplementedError(f"PLEHead: num_levels 1 or 2, got {num_levels}")
        if ns + nsh > N.PLE_MAX_OWN:
            raise NotImplementedError(f"PLEHead: specific + shared experts at most {N.PLE_MAX_OWN}, got {ns + nsh}")
        if levels == 2 and T * ns + nsh > N.PLE_MAX_SHARED_SCORES:
            raise NotImplementedError(f"PLEHead: num_tasks * specific + shared experts at most {N.PLE_MAX_SHARED_SCORES} under the "
                                      f"level-0 shared gate, got {T * ns + nsh}")
        ex, ga, to = ([int(u) for u in units] for units in (expert_dnn_hidden_units, gate_dnn_hidden_units, tower_dnn_hidden_units))
        if not 1 <= len(ex) <= N.PLE_MAX_HIDDEN:
            raise NotImplementedError(f"PLEHead: 1 to {N.PLE_MAX_HIDDEN} expert hidden layers, got {len(ex)}")
        if len(ga) > N.PLE_MAX_HIDDEN or len(to) > N.PLE_MAX_HIDDEN:
            raise NotImplementedError(f"PLEHead: 0 to {N.PLE_MAX_HIDDEN} gate and tower hidden layers, got {len(ga)} and {len(to)}")
        if inputs_dim < 1 or min(ex + ga + to) < 1:
            raise ValueError("PLEHead: inputs_dim and the hidden units must be positive")
        self.inputs_dim, self.num_tasks, self.num_levels = int(inputs_dim), T, levels
        self.shared_expert_num, self.specific_expert_num = nsh, ns
        self.expert_dnn_hidden_units, self.gate_dnn_hidden_units, self.tower_dnn_hidden_units = tuple(ex), tuple(ga), tuple(to)
        dim = lambda level: self.inputs_dim if level == 0 else ex[-1]      # noqa: E731
        gate_in = lambda level: ga[-1] if ga else dim(level)      # noqa: E731
        many = lambda level, tasks, count, units: nn.ModuleList(      # noqa: E731
            [nn.ModuleList([_TowerDNN(dim(level), units, init_std) for _ in range(count)]) for _ in range(tasks)])
        # (first: in the reference's state_dict `out.*` precedes PLE's own modules, because its BaseModel registers that name)
        self.out = nn.ModuleList([_OutBias() for _ in range(T)])
        self.specific_experts = nn.ModuleList([many(level, T, ns, ex) for level in range(levels)])
        self.shared_experts = nn.ModuleList([many(level, 1, ns, ex) for level in range(levels)])      # ns of them: the reference's
        if ga:
            self.specific_gate_dnn = nn.ModuleList([many(level, T, 1, ga) for level in range(levels)])
        self.specific_gate_dnn_final_layer = nn.ModuleList(
            [nn.ModuleList([nn.Linear(gate_in(level), ns + nsh, bias=False) for _ in range(T)]) for level in range(levels)])
        if ga:
            self.shared_gate_dnn = nn.ModuleList([_TowerDNN(dim(level), ga, init_std) for level in range(levels)])
        self.shared_gate_dnn_final_layer = nn.ModuleList(
            [nn.Linear(gate_in(level), T * ns + nsh, bias=False) for level in range(levels)])
        if to:
            self.tower_dnn = nn.ModuleList([_TowerDNN(ex[-1], to, init_std) for _ in range(T)])
        self.tower_dnn_final_layer = nn.ModuleList([nn.Linear(to[-1] if to else ex[-1], 1, bias=False) for _ in range(T)])
        self.last_gates = self.last_mixture = None

    def forward(self, dnn_input, domain_ids, domain_id_offset=0):
        x = dnn_input
        if x.dim() != 2 or x.shape[1] != self.inputs_dim:
            raise ValueError(f"PLEHead: expected input [B, {self.inputs_dim}], got {tuple(x.shape)}")
        N.require_gpu(x, "PLEHead")
        if x.dtype != torch.float32 or self.out[0].bias.dtype != torch.float32:
            raise TypeError("PLEHead: rows, parameters and gradients are float32")
        T, ns, nsh, levels = self.num_tasks, self.specific_expert_num, self.shared_expert_num, self.num_levels
        order, seg, _ = _bucket_rows(x, domain_ids, T, domain_id_offset, "PLEHead")
        task = (domain_ids.reshape(-1).to(device=x.device, dtype=torch.int64) - int(domain_id_offset)).to(torch.int32).contiguous()
        nx, ng, nt = len(self.expert_dnn_hidden_units), len(self.gate_dnn_hidden_units), len(self.tower_dnn_hidden_units)

        def stacked(dnns, n):
            layers = [[m.linears[l] for m in dnns] for l in range(n)]
            return ([torch.stack([m.weight for m in layer]) for layer in layers] +
                    [torch.stack([m.bias for m in layer]) for layer in layers])

        def specific(level):
            return [m for per_task in self.specific_experts[level] for m in per_task]

        def shared(level):
            return list(self.shared_experts[level][0])[:nsh]

        def own_gate(level):
            gate = stacked([self.specific_gate_dnn[level][t][0] for t in range(T)], ng) if ng else []
            return gate + [torch.stack([m.weight for m in self.specific_gate_dnn_final_layer[level]])]

        tensors = []
        if levels == 2:
            tensors += stacked(specific(0) + shared(0), nx) + own_gate(0)
            if ng:
                lin = self.shared_gate_dnn[0].linears
                tensors += [m.weight for m in lin] + [m.bias for m in lin]
            tensors.append(self.shared_gate_dnn_final_layer[0].weight)
        last = levels - 1
        tensors += stacked(specific(last), nx) + stacked(shared(last), nx) + own_gate(last)
        tensors += (stacked(self.tower_dnn, nt) if nt else []) + [torch.stack([m.weight for m in self.tower_dnn_final_layer]),
                                                                  torch.cat([m.bias for m in self.out])]
        widths = (self.expert_dnn_hidden_units, self.gate_dnn_hidden_units, self.tower_dnn_hidden_units)
        logit, saved = _PLEFn.apply(x, order, seg, task, (levels, ns, nsh, nx, ng, nt), widths, T, *tensors)
        B, E, n = x.shape[0], ns + nsh, self.expert_dnn_hidden_units[-1]
        self.last_gates = saved[:B * E].view(B, E)
        self.last_mixture = saved[B * E:B * (E + n)].view(B, n)
        return logit


def _sharedbottom_fill(tgt, cfg, tensors):
    """Set the parameter pointers of a satrans_sharedbottom_desc / satrans_sharedbottom_grads from `tensors`, which hold, in the
    order of N.SHAREDBOTTOM_POINTERS: bottom weights, bottom biases, tower weights, tower biases (stacked over the tasks), the
    towers' final weight, the out biases."""
    nb, nt = cfg
    it = iter(tensors)
    for name, per_layer in N.SHAREDBOTTOM_POINTERS:
        if per_layer:
            for l in range(nb if name.startswith("bottom") else nt):
                getattr(tgt, name)[l] = next(it).data_ptr()
        else:
            setattr(tgt, name, next(it).data_ptr())
    return tgt


def _sharedbottom_desc(x, order, seg, cfg, tensors):
    nb, nt = cfg
    d = _sharedbottom_fill(N.SharedBottomDesc(), cfg, tensors)
    d.B, d.C, d.T, d.n_bottom, d.n_tower = x.shape[0], x.shape[1], tensors[-1].shape[0], nb, nt
    d.x, d.order, d.seg = x.data_ptr(), order.data_ptr(), seg.data_ptr()
    for l in range(nb):
        d.bottom_width[l] = tensors[l].shape[0]
    for l in range(nt):
        d.tower_width[l] = tensors[2 * nb + l].shape[1]
    return d


class _SharedBottomFn(torch.autograd.Function):
    """logit [B,1] of the scenario-routed SharedBottom head (csrc/sharedbottom.hip); `tensors` as _sharedbottom_fill lists them."""

    @staticmethod
    def forward(ctx, x, order, seg, cfg, *tensors):
        lib = N.lib()
        dev = x.device
        x = x.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        d = _sharedbottom_desc(x, order, seg, cfg, tensors)
        saved = torch.empty(_native_size(lib.satrans_sharedbottom_saved_floats, d), dtype=torch.float32, device=dev)
        logit = torch.empty(x.shape[0], 1, dtype=torch.float32, device=dev)
        N.check(lib.satrans_sharedbottom_fwd(C.byref(d), logit.data_ptr(), saved.data_ptr(), N.stream_handle(dev)),
                "satrans_sharedbottom_fwd")
        ctx.cfg = cfg
        ctx.save_for_backward(x, order, seg, saved, *tensors)
        ctx.mark_non_differentiable(saved)
        return logit, saved

    @staticmethod
    def backward(ctx, dlogit, _dsaved):
        lib = N.lib()
        x, order, seg, saved, *tensors = ctx.saved_tensors
        d = _sharedbottom_desc(x, order, seg, ctx.cfg, tensors)
        work = torch.empty(_native_size(lib.satrans_sharedbottom_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(t) for t in tensors]
        g = _sharedbottom_fill(N.SharedBottomGrads(), ctx.cfg, grads)
        N.check(lib.satrans_sharedbottom_bwd(C.byref(d), dlogit.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(),
                                             work.data_ptr(), C.byref(g), N.stream_handle(x.device)), "satrans_sharedbottom_bwd")
        return (dx, None, None, None, *grads)


class SharedBottomHead(nn.Module):
    """The bottom / tower half of the reference's SharedBottom.forward (models/sharedbottom.py:120-133) over a mixed batch, for
    the reference's one-task-per-scenario use (T = tasks = scenarios): the loss of mtl_basemodel.py:268-269 and predict
    (:376-378) read, of a row's T outputs, only the column of the row's own scenario.  So the bottom DNN runs over all rows, and
    a row whose id is t + domain_id_offset goes through task t's tower DNN, tower_dnn_final_layer and out[t].bias - nothing of
    the other tasks.

    Parameter names, shapes, state_dict order and initialisation are the reference SharedBottom's (DNN weights N(0, init_std),
    their biases and the bias-free final nn.Linears torch's default, out.{t}.bias zeros): out.{t}.bias,
    bottom_dnn.linears.{l}.*, tower_dnn.{t}.linears.{l}.* (only with tower hidden units), tower_dnn_final_layer.{t}.weight -
    those entries of a reference checkpoint load with load_state_dict.

    forward(dnn_input [B, inputs_dim] fp32, domain_ids [B], domain_id_offset=0) -> logit [B,1]; the caller applies the
    sigmoid.  Per call: the ids are bucketed once (one device-to-host read), the per-task parameters stacked (torch.stack;
    autograd splits the gradients back), and one autograd.Function runs satrans_sharedbottom_fwd / satrans_sharedbottom_bwd.
    `last_bottom` [B, last bottom width] is a view of the last forward's saved buffer: the shared bottom's output.

    Differences from the reference.  (1) The module returns each row's OWN task logit, [B,1], not the [B,T] matrix of all
    tasks: the other T - 1 columns are never computed.  (2) l2_reg_dnn is not applied (main.py leaves it 0).  (3) An id
    outside [offset, offset + num_tasks) raises IndexError; the reference's loss silently leaves such rows out.
    Not built - NotImplementedError at construction: an activation other than relu, dropout, batch-norm inside the DNNs,
    no bottom layer, more than 3 hidden layers in a DNN."""

    def __init__(self, inputs_dim, num_tasks, bottom_dnn_hidden_units=(256, 128), tower_dnn_hidden_units=(64,), init_std=0.0001,
                 dnn_activation='relu', dnn_dropout=0, dnn_use_bn=False):
        super().__init__()
        if dnn_activation != 'relu':
            raise NotImplementedError(f"SharedBottomHead: activation {dnn_activation!r} is not built (relu only)")
        if dnn_dropout != 0:
            raise NotImplementedError("SharedBottomHead: dropout inside the DNNs is not built (dnn_dropout must be 0)")
        if dnn_use_bn:
            raise NotImplementedError("SharedBottomHead: batch-norm inside the DNNs is not built (dnn_use_bn must be False)")
        if num_tasks <= 1:
            raise ValueError("num_tasks must be greater than 1")
        bo, to = ([int(u) for u in units] for units in (bottom_dnn_hidden_units, tower_dnn_hidden_units))
        if not 1 <= len(bo) <= N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"SharedBottomHead: 1 to {N.MMOE_MAX_HIDDEN} bottom hidden layers, got {len(bo)}")
        if len(to) > N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"SharedBottomHead: 0 to {N.MMOE_MAX_HIDDEN} tower hidden layers, got {len(to)}")
        if inputs_dim < 1 or min(bo + to) < 1:
            raise ValueError("SharedBottomHead: inputs_dim and the hidden units must be positive")
        self.inputs_dim, self.num_tasks = int(inputs_dim), int(num_tasks)
        self.bottom_dnn_hidden_units, self.tower_dnn_hidden_units = tuple(bo), tuple(to)
        T = self.num_tasks
        # (first: in the reference's state_dict `out.*` precedes SharedBottom's own modules, because its BaseModel registers that name)
        self.out = nn.ModuleList([_OutBias() for _ in range(T)])
        self.bottom_dnn = _TowerDNN(inputs_dim, bo, init_std)
        if to:
            self.tower_dnn = nn.ModuleList([_TowerDNN(bo[-1], to, init_std) for _ in range(T)])
        self.tower_dnn_final_layer = nn.ModuleList([nn.Linear(to[-1] if to else bo[-1], 1, bias=False) for _ in range(T)])
        self.last_bottom = None

    def forward(self, dnn_input, domain_ids, domain_id_offset=0):
        x = dnn_input
        if x.dim() != 2 or x.shape[1] != self.inputs_dim:
            raise ValueError(f"SharedBottomHead: expected input [B, {self.inputs_dim}], got {tuple(x.shape)}")
        N.require_gpu(x, "SharedBottomHead")
        if x.dtype != torch.float32 or self.out[0].bias.dtype != torch.float32:
            raise TypeError("SharedBottomHead: rows, parameters and gradients are float32")
        order, seg, _ = _bucket_rows(x, domain_ids, self.num_tasks, domain_id_offset, "SharedBottomHead")
        bo, nt = self.bottom_dnn_hidden_units, len(self.tower_dnn_hidden_units)
        tensors = [m.weight for m in self.bottom_dnn.linears] + [m.bias for m in self.bottom_dnn.linears]
        if nt:
            layers = [[m.linears[l] for m in self.tower_dnn] for l in range(nt)]
            tensors += ([torch.stack([m.weight for m in layer]) for layer in layers] +
                        [torch.stack([m.bias for m in layer]) for layer in layers])
        tensors += [torch.stack([m.weight for m in self.tower_dnn_final_layer]), torch.cat([m.bias for m in self.out])]
        logit, saved = _SharedBottomFn.apply(x, order, seg, (len(bo), nt), *tensors)
        B, at = x.shape[0], x.shape[0] * sum(bo[:-1])
        self.last_bottom = saved[at:at + B * bo[-1]].view(B, bo[-1])
        return logit


def _adasparse_fill(tgt, L, tensors):
    """Set the parameter pointers of a satrans_adasparse_desc / satrans_adasparse_grads from `tensors`: L linears weights, L
    linears biases, L pruners weights, L pruners biases and, for the head, dnn_linear.weight and out.bias."""
    it = iter(tensors)
    for name, per_layer in N.ADASPARSE_POINTERS:
        if per_layer:
            for l in range(L):
                getattr(tgt, name)[l] = next(it).data_ptr()
        elif len(tensors) > 4 * L:
            setattr(tgt, name, next(it).data_ptr())
    return tgt


def _adasparse_desc(x, emb, consts, L, tensors):
    d = _adasparse_fill(N.AdaSparseDesc(), L, tensors)
    d.B, d.C, d.E, d.n_layers = x.shape[0], x.shape[1], emb.shape[1], L
    for l in range(L):
        d.width[l] = tensors[l].shape[0]
    d.alpha, d.beta, d.epsilon = consts
    d.x, d.emb = x.data_ptr(), emb.data_ptr()
    return d


class _AdaSparseFn(torch.autograd.Function):
    """The pruned DNN (csrc/adasparse.hip) over x [B,C] and the rows' scenario embeddings emb [B,E]; `tensors` as
    _adasparse_fill lists them.  With the two head tensors the first output is the logit [B,1], without them h_L [B, n_L]."""

    @staticmethod
    def forward(ctx, x, emb, consts, L, *tensors):
        lib = N.lib()
        dev = x.device
        x, emb = x.contiguous(), emb.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        d = _adasparse_desc(x, emb, consts, L, tensors)
        saved = torch.empty(_native_size(lib.satrans_adasparse_saved_floats, d), dtype=torch.float32, device=dev)
        head = len(tensors) > 4 * L
        B, n_last = x.shape[0], tensors[L - 1].shape[0]
        logit = torch.empty(B, 1, dtype=torch.float32, device=dev) if head else None
        N.check(lib.satrans_adasparse_fwd(C.byref(d), logit.data_ptr() if head else None, saved.data_ptr(), N.stream_handle(dev)),
                "satrans_adasparse_fwd")
        ctx.consts, ctx.L = consts, L
        ctx.save_for_backward(x, emb, saved, *tensors)
        ctx.mark_non_differentiable(saved)
        if head:
            return logit, saved
        at = sum(3 * B * t.shape[0] for t in tensors[:L]) - B * n_last      # h_L: the last block of the last layer
        return saved[at:at + B * n_last].view(B, n_last).clone(), saved

    @staticmethod
    def backward(ctx, dout, _dsaved):
        lib = N.lib()
        x, emb, saved, *tensors = ctx.saved_tensors
        d = _adasparse_desc(x, emb, ctx.consts, ctx.L, tensors)
        work = torch.empty(_native_size(lib.satrans_adasparse_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx, demb = torch.empty_like(x), torch.empty_like(emb)
        grads = [torch.empty_like(t) for t in tensors]
        g = _adasparse_fill(N.AdaSparseGrads(), ctx.L, grads)
        N.check(lib.satrans_adasparse_bwd(C.byref(d), dout.contiguous().data_ptr(), dx.data_ptr(), demb.data_ptr(), saved.data_ptr(),
                                          work.data_ptr(), C.byref(g), N.stream_handle(x.device)), "satrans_adasparse_bwd")
        return (dx, demb, None, None, *grads)


class PrunedDNN(nn.Module):
    """AdaSparse's DNN with a scenario-aware pruner beside every layer - a drop-in for the reference's DNN_w_Pruner
    (models/adasparse.py:28-106) as main.py configures it (relu, no dropout, no batch-norm).  Layer l computes

        fc = linears[l](h),   pi = beta * sigmoid(alpha * pruners[l](cat([h, domain_embs], 1))),   pi[|pi| - epsilon <= 0] = 0,
        h  = relu(fc * pi)

    as ONE launch (both products over one staged row tile; the concatenation is never built).  Nothing is routed: every row
    uses the same weights, the scenario enters through `domain_embs` only.  Parameters `linears.{l}.*` then `pruners.{l}.*`
    with the reference's shapes and initialisation (linears weights N(0, init_std), everything else torch's default);
    `alpha`, `beta`, `epsilon` are plain attributes as in the reference (1, 2.0, 0.25) and are read at every call.

    forward(inputs [B, inputs_dim] fp32, domain_embs [B, domain_emb_dim] fp32) -> [B, hidden_units[-1]]; gradients flow to
    both inputs.  `last_pi` is a list of [B, n_l] views of the last forward's saved buffer: the pruned factors, exactly 0
    where a unit was pruned.

    Not built - NotImplementedError at construction: an activation other than relu, dropout, use_bn, more than 3 hidden
    layers.  ValueError for empty or non-positive widths.  beta must be positive and epsilon non-negative (ValueError at call)."""

    def __init__(self, inputs_dim, hidden_units, domain_emb_dim=32, init_std=0.0001, activation='relu', dropout_rate=0, use_bn=False):
        super().__init__()
        what = type(self).__name__
        if activation != 'relu':
            raise NotImplementedError(f"{what}: activation {activation!r} is not built (relu only)")
        if dropout_rate != 0:
            raise NotImplementedError(f"{what}: dropout inside the DNN is not built (dropout_rate must be 0)")
        if use_bn:
            raise NotImplementedError(f"{what}: batch-norm inside the DNN is not built (use_bn must be False)")
        hidden_units = [int(u) for u in hidden_units]
        if len(hidden_units) == 0:
            raise ValueError("hidden_units is empty!!")
        if len(hidden_units) > N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"{what}: 1 to {N.MMOE_MAX_HIDDEN} hidden layers, got {len(hidden_units)}")
        if inputs_dim < 1 or domain_emb_dim < 1 or min(hidden_units) < 1:
            raise ValueError(f"{what}: inputs_dim, domain_emb_dim and hidden_units must be positive")
        self.inputs_dim, self.hidden_units, self.domain_emb_dim = int(inputs_dim), tuple(hidden_units), int(domain_emb_dim)
        units = [self.inputs_dim] + hidden_units
        self.linears = nn.ModuleList([nn.Linear(units[i], units[i + 1]) for i in range(len(units) - 1)])
        self.pruners = nn.ModuleList([nn.Linear(units[i] + self.domain_emb_dim, units[i + 1]) for i in range(len(units) - 1)])
        for lin in self.linears:
            nn.init.normal_(lin.weight, mean=0, std=init_std)
        self.beta, self.epsilon, self.alpha = 2.0, 0.25, 1
        self.last_pi = None

    def _check(self, x, emb, what):
        if x.dim() != 2 or x.shape[1] != self.inputs_dim:
            raise ValueError(f"{what}: expected input [B, {self.inputs_dim}], got {tuple(x.shape)}")
        if emb.dim() != 2 or emb.shape[1] != self.domain_emb_dim or emb.shape[0] != x.shape[0]:
            raise ValueError(f"{what}: expected domain embeddings [{x.shape[0]}, {self.domain_emb_dim}], got {tuple(emb.shape)}")
        N.require_gpu(x, what)
        N.require_gpu(emb, what)
        if x.dtype != torch.float32 or emb.dtype != torch.float32 or self.linears[0].weight.dtype != torch.float32:
            raise TypeError(f"{what}: rows, parameters and gradients are float32")
        if not (self.beta > 0 and self.epsilon >= 0):
            raise ValueError(f"{what}: beta must be positive and epsilon non-negative, got {self.beta} and {self.epsilon}")

    def _run(self, x, emb, head=()):
        L = len(self.hidden_units)
        tensors = ([m.weight for m in self.linears] + [m.bias for m in self.linears] + [m.weight for m in self.pruners] +
                   [m.bias for m in self.pruners] + list(head))
        out, saved = _AdaSparseFn.apply(x, emb, (float(self.alpha), float(self.beta), float(self.epsilon)), L, *tensors)
        B, at, self.last_pi = x.shape[0], 0, []
        for n in self.hidden_units:      # saved, per layer: pi, dzf, h
            self.last_pi.append(saved[at:at + B * n].view(B, n))
            at += 3 * B * n
        return out

    def forward(self, inputs, domain_embs):
        self._check(inputs, domain_embs, "PrunedDNN")
        return self._run(inputs, domain_embs)


class AdaSparseHead(nn.Module):
    """The part of the reference's AdaSparse.forward after the embeddings (models/adasparse.py:185-189): the pruned DNN, the
    bias-free dnn_linear and the bias of the prediction layer.  state_dict keys and order are the reference's - out.bias,
    dnn.linears.{l}.*, dnn.pruners.{l}.*, dnn_linear.weight - so those entries of a reference checkpoint load with
    load_state_dict.  `dnn` is a PrunedDNN; set alpha, beta, epsilon there; `last_pi` is its.

    forward(dnn_input [B, inputs_dim] fp32, domain_emb [B, domain_emb_dim] fp32) -> logit [B,1]; the caller applies the
    sigmoid.  One autograd.Function runs the whole stack (satrans_adasparse_fwd / satrans_adasparse_bwd); gradients flow to
    both inputs, so a `domain_emb` gathered from the model's own embedding table gives the table both of its gradient paths.

    Differences from the reference.  (1) domain_emb must be [B, E]: the reference's `.squeeze()` turns a batch of one row into
    [E] and then fails in its torch.cat; that quirk is not reproduced.  (2) l2_reg_dnn is not applied (main.py leaves it 0).
    Not built: what PrunedDNN refuses."""

    def __init__(self, inputs_dim, dnn_hidden_units=(256, 128), domain_emb_dim=32, init_std=0.0001, dnn_activation='relu',
                 dnn_dropout=0, dnn_use_bn=False):
        super().__init__()
        # (first: in the reference's state_dict `out.*` precedes AdaSparse's own modules, because its BaseModel registers that name)
        self.out = _OutBias()
        self.dnn = PrunedDNN(inputs_dim, dnn_hidden_units, domain_emb_dim=domain_emb_dim, init_std=init_std, activation=dnn_activation,
                             dropout_rate=dnn_dropout, use_bn=dnn_use_bn)
        self.dnn_linear = nn.Linear(self.dnn.hidden_units[-1], 1, bias=False)

    @property
    def last_pi(self):
        return self.dnn.last_pi

    def forward(self, dnn_input, domain_emb):
        self.dnn._check(dnn_input, domain_emb, "AdaSparseHead")
        return self.dnn._run(dnn_input, domain_emb, head=(self.dnn_linear.weight, self.out.bias))


def _cin_fill(tgt, L, tensors):
    """Set the w / b pointers of a satrans_cin_desc / satrans_cin_grads from `tensors`: the L weights, then the L biases."""
    for i in range(L):
        tgt.w[i], tgt.b[i] = tensors[i].data_ptr(), tensors[L + i].data_ptr()
    return tgt


def _cin_desc(x, split_half, tensors):
    L = len(tensors) // 2
    d = _cin_fill(N.CINDesc(), L, tensors)
    d.B, d.M, d.D, d.L, d.split_half = x.shape[0], x.shape[1], x.shape[2], L, int(split_half)
    d.x0 = x.data_ptr()
    for i in range(L):
        d.width[i] = tensors[i].shape[0]
    return d


class _CINFn(torch.autograd.Function):
    """result [B, featuremap_num] of the compressed interaction network (csrc/cin.hip); `tensors`: the Conv1d weights
    [O_i, H_i M, 1] of the layers, then their biases."""

    @staticmethod
    def forward(ctx, x, split_half, *tensors):
        lib = N.lib()
        dev = x.device
        x = x.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        d = _cin_desc(x, split_half, tensors)
        saved = torch.empty(_native_size(lib.satrans_cin_saved_floats, d), dtype=torch.float32, device=dev)
        L = len(tensors) // 2
        widths = [t.shape[0] for t in tensors[:L]]
        F = sum(w - (w // 2 if split_half and i != L - 1 else 0) for i, w in enumerate(widths))
        result = torch.empty(x.shape[0], F, dtype=torch.float32, device=dev)
        N.check(lib.satrans_cin_fwd(C.byref(d), result.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_cin_fwd")
        ctx.split_half = split_half
        ctx.save_for_backward(x, saved, *tensors)
        ctx.mark_non_differentiable(saved)
        return result, saved

    @staticmethod
    def backward(ctx, dresult, _dsaved):
        lib = N.lib()
        x, saved, *tensors = ctx.saved_tensors
        d = _cin_desc(x, ctx.split_half, tensors)
        work = torch.empty(_native_size(lib.satrans_cin_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(t) for t in tensors]
        g = _cin_fill(N.CINGrads(), len(tensors) // 2, grads)
        N.check(lib.satrans_cin_bwd(C.byref(d), dresult.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                    C.byref(g), N.stream_handle(x.device)), "satrans_cin_bwd")
        return (dx, None, *grads)


class CIN(nn.Module):
    """deepctr-torch's Compressed Interaction Network, the interaction layer of the reference's xDeepFM (models/xdeepfm.py:73,
    96-98), with deepctr's constructor: `l2_reg`, `seed` and `device` are accepted and unused.  With X0 = inputs [B, M, D] and
    X_0 = X0, layer i is `relu(Conv1d(H_i M, O_i, 1)(outer(X_i, X0)))` over the [B, H_i M, D] outer product along the fields;
    under split_half the first half of a layer's channels feeds the next layer and the second half is output, the last layer is
    output whole; the output channels of all layers, summed over D, make the result.

    forward(inputs [B, field_size, D] fp32 on the GPU) -> [B, featuremap_num].  The outer product is never materialised: the
    kernels form its elements from the two factors while the weights stream (csrc/cin.hip), forward and backward, so the memory
    a call needs is the layers' activations [B, O_i, D].  One autograd.Function runs satrans_cin_fwd / satrans_cin_bwd.

    Parameters are deepctr's, `conv1ds.{i}.weight` [O_i, H_i M, 1] and `conv1ds.{i}.bias` [O_i] with torch's Conv1d default
    initialisation: the `cin.conv1ds.*` entries of a reference xDeepFM checkpoint load with load_state_dict.
    Not built - NotImplementedError at construction: an activation other than relu, more than CIN_MAX_LAYERS layers, more
    than CIN_MAX_FIELDS fields, a layer wider than CIN_MAX_WIDTH.  l2_reg is not applied (main.py leaves l2_reg_cin 0)."""

    def __init__(self, field_size, layer_size=(128, 128), activation='relu', split_half=True, l2_reg=1e-5, seed=1024, device='cpu'):
        super().__init__()
        if len(layer_size) == 0:
            raise ValueError("layer_size must be a list(tuple) of length greater than 1")
        if activation != 'relu':
            raise NotImplementedError(f"CIN: activation {activation!r} is not built (relu only)")
        sizes = [int(s) for s in layer_size]
        if field_size < 1 or min(sizes) < 1:
            raise ValueError("CIN: field_size and the layer sizes must be positive")
        if len(sizes) > N.CIN_MAX_LAYERS:
            raise NotImplementedError(f"CIN: 1 to {N.CIN_MAX_LAYERS} layers, got {len(sizes)}")
        if field_size > N.CIN_MAX_FIELDS:
            raise NotImplementedError(f"CIN: 1 to {N.CIN_MAX_FIELDS} fields, got {field_size}")
        if max(sizes) > N.CIN_MAX_WIDTH:
            raise NotImplementedError(f"CIN: layer sizes up to {N.CIN_MAX_WIDTH}, got {max(sizes)}")
        self.layer_size, self.split_half, self.activation = tuple(sizes), bool(split_half), activation
        self.field_nums = [int(field_size)]
        self.conv1ds = nn.ModuleList()
        for i, size in enumerate(sizes):
            self.conv1ds.append(nn.Conv1d(self.field_nums[-1] * self.field_nums[0], size, 1))
            if self.split_half:
                if i != len(sizes) - 1 and size % 2 > 0:
                    raise ValueError("layer_size must be even number except for the last layer when split_half=True")
                self.field_nums.append(size // 2)
            else:
                self.field_nums.append(size)
        self.featuremap_num = sum(sizes[:-1]) // 2 + sizes[-1] if self.split_half else sum(sizes)

    def forward(self, inputs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        if inputs.shape[1] != self.field_nums[0]:
            raise ValueError(f"CIN: expected inputs [B, {self.field_nums[0]}, D], got {tuple(inputs.shape)}")
        N.require_gpu(inputs, "CIN")
        if inputs.dtype != torch.float32 or self.conv1ds[0].weight.dtype != torch.float32:
            raise TypeError("CIN: inputs, parameters and gradients are float32")
        tensors = [c.weight for c in self.conv1ds] + [c.bias for c in self.conv1ds]
        result, _ = _CINFn.apply(inputs, self.split_half, *tensors)
        return result


class XDeepFMHead(nn.Module):
    """The half of the reference's xDeepFM.forward behind the embedding lookup (models/xdeepfm.py:94-115):

        logit = linear_logit + cin_linear(cin(emb)) + dnn_linear(dnn(cat(flatten(emb), dense))) + out.bias

    forward(emb [B, field_size, embedding_size] fp32, dense [B, dense_dim] or None, linear_logit [B,1] or None) -> logit [B,1];
    the caller applies the sigmoid.  `emb` is the concatenation of the looked-up sparse embeddings in field order; the
    reference's `metatrans` flag (xdeepfm.py:87-90) transforms that block first, which here is

        head = XDeepFMHead(F, D, dense_dim, ...); meta = MetaTransformation(D, num_domains)
        logit = head(meta(domain_ids, emb), dense, linear_logit)

    The CIN - 25.8 of xDeepFM's 26.3 MFLOP per sample at the AliCCP shape - is `CIN` above (csrc/cin.hip).  The DNN branch
    (Linear + relu layers) and the two one-column Linears are plain torch modules: under 2 % of the FLOPs.  Empty
    dnn_hidden_units or an empty cin_layer_size drops that branch, as the reference does.

    Parameter names, shapes, state_dict order and initialisation are the reference xDeepFM's: out.bias (zeros),
    dnn.linears.{l}.{weight,bias} (weights N(0, init_std)), dnn_linear.weight, cin.conv1ds.{i}.{weight,bias}, cin_linear.weight
    - those entries of a reference checkpoint load with load_state_dict.
    Not built, as in the other heads: l2_reg_*, dropout, batch-norm, activations other than relu."""

    def __init__(self, field_size, embedding_size, dense_dim=0, dnn_hidden_units=(256, 256), cin_layer_size=(256, 128),
                 cin_split_half=True, init_std=0.0001):
        super().__init__()
        if field_size < 1 or embedding_size < 1 or dense_dim < 0:
            raise ValueError("XDeepFMHead: field_size and embedding_size must be positive, dense_dim non-negative")
        self.field_size, self.embedding_size, self.dense_dim = int(field_size), int(embedding_size), int(dense_dim)
        units = [int(u) for u in dnn_hidden_units]
        self.use_dnn, self.use_cin = len(units) > 0, len(cin_layer_size) > 0
        # (first: in the reference's state_dict `out.*` precedes xDeepFM's own modules, because its BaseModel registers that name)
        self.out = _OutBias()
        if self.use_dnn:
            self.dnn = _TowerDNN(self.field_size * self.embedding_size + self.dense_dim, units, init_std)
            self.dnn_linear = nn.Linear(units[-1], 1, bias=False)
        if self.use_cin:
            self.cin = CIN(field_size, cin_layer_size, 'relu', cin_split_half)
            self.featuremap_num = self.cin.featuremap_num
            self.cin_linear = nn.Linear(self.featuremap_num, 1, bias=False)

    def forward(self, emb, dense=None, linear_logit=None):
        if emb.dim() != 3 or emb.shape[1] != self.field_size or emb.shape[2] != self.embedding_size:
            raise ValueError(f"XDeepFMHead: expected emb [B, {self.field_size}, {self.embedding_size}], got {tuple(emb.shape)}")
        got = 0 if dense is None else (dense.shape[1] if dense.dim() == 2 else -1)
        if got != self.dense_dim:
            raise ValueError(f"XDeepFMHead: expected dense [B, {self.dense_dim}], got "
                             f"{None if dense is None else tuple(dense.shape)}")
        N.require_gpu(emb, "XDeepFMHead")
        if emb.dtype != torch.float32:
            raise TypeError("XDeepFMHead: rows, parameters and gradients are float32")
        logit = linear_logit      # the reference's order of the sum: linear + dnn + cin, then the bias of `out`
        if self.use_dnn:
            h = torch.flatten(emb, start_dim=1)
            if dense is not None:
                h = torch.cat([h, dense], dim=-1)
            for lin in self.dnn.linears:
                h = torch.relu(lin(h))
            h = self.dnn_linear(h)
            logit = h if logit is None else logit + h
        if self.use_cin:
            h = self.cin_linear(self.cin(emb))
            logit = h if logit is None else logit + h
        if logit is None:
            return self.out.bias.reshape(1, 1).expand(emb.shape[0], 1)
        return logit + self.out.bias


def _cross_desc(x, matrix, kernels, bias):
    d = N.CrossDesc()
    d.B, d.N, d.L, d.matrix = x.shape[0], x.shape[1], kernels.shape[0], int(matrix)
    d.x0, d.kernels, d.bias = x.data_ptr(), kernels.data_ptr(), bias.data_ptr()
    return d


class _CrossFn(torch.autograd.Function):
    """result [B, N] of the cross network (csrc/cross.hip); kernels [L, N, 1] (vector form) or [L, N, N] (matrix form), bias
    [L, N, 1].  `saved` is what the backward keeps: [B L] in the vector form, [(2 L - 1) B N] in the matrix form."""

    @staticmethod
    def forward(ctx, x, matrix, kernels, bias):
        lib = N.lib()
        dev = x.device
        x, kernels, bias = x.contiguous(), kernels.contiguous(), bias.contiguous()
        d = _cross_desc(x, matrix, kernels, bias)
        saved = torch.empty(_native_size(lib.satrans_cross_saved_floats, d), dtype=torch.float32, device=dev)
        result = torch.empty_like(x)
        N.check(lib.satrans_cross_fwd(C.byref(d), result.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_cross_fwd")
        ctx.matrix = matrix
        ctx.save_for_backward(x, saved, kernels, bias)
        ctx.mark_non_differentiable(saved)
        return result, saved

    @staticmethod
    def backward(ctx, dresult, _dsaved):
        lib = N.lib()
        x, saved, kernels, bias = ctx.saved_tensors
        d = _cross_desc(x, ctx.matrix, kernels, bias)
        work = torch.empty(_native_size(lib.satrans_cross_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx, dk, db = torch.empty_like(x), torch.empty_like(kernels), torch.empty_like(bias)
        g = N.CrossGrads()
        g.kernels, g.bias = dk.data_ptr(), db.data_ptr()
        N.check(lib.satrans_cross_bwd(C.byref(d), dresult.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                      C.byref(g), N.stream_handle(x.device)), "satrans_cross_bwd")
        return dx, None, dk, db


class CrossNet(nn.Module):
    """deepctr-torch's cross network, which the reference's DCN calls (models/dcn.py:70,101), with deepctr's constructor: `seed`
    and `device` are accepted and unused.  With x_0 = inputs [B, N]:

        vector:  x_{l+1} = x_0 (x_l . kernels[l]) + bias[l] + x_l               kernels [L, N, 1]
        matrix:  x_{l+1} = x_0 * (kernels[l] x_l + bias[l]) + x_l               kernels [L, N, N]

    forward(inputs [B, in_features] fp32 on the GPU) -> [B, in_features].  One autograd.Function runs satrans_cross_fwd /
    satrans_cross_bwd (csrc/cross.hip).  The vector form is one launch for the whole stack each way and keeps B L scalars for the
    backward, not the layer inputs; the matrix form is a tile product per layer on the exact f32-input MFMA.
    layer_num = 0 keeps the zero-length parameters and returns the input.

    Parameters are deepctr's, `kernels` and `bias` [L, N, 1], with its initialisation in its order (xavier_normal_ of each
    kernels[i], zeros for the bias): the `crossnet.*` entries of a reference DCN checkpoint load with load_state_dict.
    Not built - NotImplementedError at construction: more than CROSS_MAX_LAYERS layers, more than CROSS_MAX_FEATURES features."""

    def __init__(self, in_features, layer_num=2, parameterization='vector', seed=1024, device='cpu'):
        super().__init__()
        if parameterization not in ('vector', 'matrix'):
            raise ValueError("parameterization should be 'vector' or 'matrix'")
        in_features, layer_num = int(in_features), int(layer_num)
        if in_features < 1 or layer_num < 0:
            raise ValueError("CrossNet: in_features must be positive and layer_num non-negative")
        if layer_num > N.CROSS_MAX_LAYERS:
            raise NotImplementedError(f"CrossNet: up to {N.CROSS_MAX_LAYERS} layers, got {layer_num}")
        if in_features > N.CROSS_MAX_FEATURES:
            raise NotImplementedError(f"CrossNet: up to {N.CROSS_MAX_FEATURES} features, got {in_features}")
        self.in_features, self.layer_num, self.parameterization = in_features, layer_num, parameterization
        self.kernels = nn.Parameter(torch.empty(layer_num, in_features, 1 if parameterization == 'vector' else in_features))
        self.bias = nn.Parameter(torch.empty(layer_num, in_features, 1))
        for i in range(layer_num):
            nn.init.xavier_normal_(self.kernels[i])
        for i in range(layer_num):
            nn.init.zeros_(self.bias[i])

    def forward(self, inputs):
        if inputs.dim() != 2 or inputs.shape[1] != self.in_features:
            raise ValueError(f"CrossNet: expected inputs [B, {self.in_features}], got {tuple(inputs.shape)}")
        N.require_gpu(inputs, "CrossNet")
        if inputs.dtype != torch.float32 or self.kernels.dtype != torch.float32:
            raise TypeError("CrossNet: inputs, parameters and gradients are float32")
        if self.layer_num == 0:
            return inputs
        result, _ = _CrossFn.apply(inputs, self.parameterization == 'matrix', self.kernels, self.bias)
        return result


class DCNHead(nn.Module):
    """The half of the reference's DCN.forward behind the embedding lookup (models/dcn.py:90-113), with dnn_input =
    cat(flatten(emb), dense):

        logit = linear_logit + dnn_linear(cat(crossnet(dnn_input), dnn(dnn_input))) + out.bias      (deep & cross)
                             + dnn_linear(dnn(dnn_input))                                            (cross_num = 0)
                             + dnn_linear(crossnet(dnn_input))                                       (dnn_hidden_units = ())

    forward(emb [B, field_size, embedding_size] fp32, dense [B, dense_dim] or None, linear_logit [B,1] or None) -> logit [B,1];
    the caller applies the sigmoid.  The reference's `metatrans` flag (dcn.py:87-88) transforms the embedding block first:

        head = DCNHead(F, D, dense_dim, ...); meta = MetaTransformation(D, num_domains)
        logit = head(meta(domain_ids, emb), dense, linear_logit)

    The cross network is `CrossNet` above (csrc/cross.hip).  The DNN (Linear + relu layers), `dnn_linear` and the two
    concatenations are plain torch modules.  At the AliCCP width N = 19 x 32 = 608 with main.py's defaults the DNN is
    2 (608 x 128 + 128 x 128) = 188 kFLOP per sample and dnn_linear 1.5 k; the vector cross network is 2 layers x 3 N = 3.6 k, so
    98 % of DCN-V's FLOPs stay in torch - its cross network is memory traffic, not arithmetic.  In DCN-M (2 layers x 2 N^2 =
    1.48 MFLOP) torch keeps 11 %.  Moving the DNN onto the dense layer launcher of csrc/head_layers.h is the next step.

    Parameter names, shapes, state_dict order and initialisation are the reference DCN's: out.bias (zeros),
    dnn.linears.{l}.{weight,bias} (weights N(0, init_std)), dnn_linear.weight, crossnet.kernels, crossnet.bias - those entries
    of a reference checkpoint load with load_state_dict.  Empty dnn_hidden_units leaves no `dnn.*` entries; cross_num = 0
    keeps the zero-length `crossnet.*` entries, as the reference does.

    regularization_loss() -> [1] is what DCN.__init__ itself adds to the reference's regularization_weight with a non-zero
    factor, l2_reg_linear sum(dnn_linear.weight^2) + l2_reg_cross sum(crossnet.kernels^2), in get_regularization_loss's
    arithmetic (main.py leaves both at 1e-5, so a port adds it to its loss).  Not built, as in the other heads: l2_reg_dnn,
    dropout, batch-norm, activations other than relu."""

    def __init__(self, field_size, embedding_size, dense_dim=0, cross_num=2, cross_parameterization='vector',
                 dnn_hidden_units=(128, 128), l2_reg_linear=1e-5, l2_reg_cross=1e-5, init_std=0.0001):
        super().__init__()
        if field_size < 1 or embedding_size < 1 or dense_dim < 0:
            raise ValueError("DCNHead: field_size and embedding_size must be positive, dense_dim non-negative")
        self.field_size, self.embedding_size, self.dense_dim = int(field_size), int(embedding_size), int(dense_dim)
        units = [int(u) for u in dnn_hidden_units]
        self.cross_num = int(cross_num)
        self.use_dnn, self.use_cross = len(units) > 0, self.cross_num > 0
        if not (self.use_dnn or self.use_cross):
            raise ValueError("DCNHead: cross_num = 0 with empty dnn_hidden_units leaves no branch")
        self.l2_reg_linear, self.l2_reg_cross = float(l2_reg_linear), float(l2_reg_cross)
        n = self.field_size * self.embedding_size + self.dense_dim
        # (first: in the reference's state_dict `out.*` precedes DCN's own modules, because its BaseModel registers that name)
        self.out = _OutBias()
        self.dnn = _TowerDNN(n, units, init_std)
        self.dnn_linear = nn.Linear((n if self.use_cross else 0) + (units[-1] if self.use_dnn else 0), 1, bias=False)
        self.crossnet = CrossNet(n, self.cross_num, cross_parameterization)

    def regularization_loss(self):
        total = torch.zeros((1,), device=self.dnn_linear.weight.device)
        for p, l2 in ((self.dnn_linear.weight, self.l2_reg_linear), (self.crossnet.kernels, self.l2_reg_cross)):
            if l2 > 0:
                total = total + torch.sum(l2 * torch.square(p))
        return total

    def forward(self, emb, dense=None, linear_logit=None):
        if emb.dim() != 3 or emb.shape[1] != self.field_size or emb.shape[2] != self.embedding_size:
            raise ValueError(f"DCNHead: expected emb [B, {self.field_size}, {self.embedding_size}], got {tuple(emb.shape)}")
        got = 0 if dense is None else (dense.shape[1] if dense.dim() == 2 else -1)
        if got != self.dense_dim:
            raise ValueError(f"DCNHead: expected dense [B, {self.dense_dim}], got "
                             f"{None if dense is None else tuple(dense.shape)}")
        N.require_gpu(emb, "DCNHead")
        if emb.dtype != torch.float32:
            raise TypeError("DCNHead: rows, parameters and gradients are float32")
        x = torch.flatten(emb, start_dim=1)
        if dense is not None:
            x = torch.cat([x, dense], dim=-1)
        parts = []
        if self.use_cross:
            parts.append(self.crossnet(x))
        if self.use_dnn:
            h = x
            for lin in self.dnn.linears:
                h = torch.relu(lin(h))
            parts.append(h)
        h = self.dnn_linear(parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1))
        logit = h if linear_logit is None else linear_logit + h
        return logit + self.out.bias


def _senet_desc(x, w1, w2):
    d = N.SENetDesc()
    d.B, d.F, d.D, d.R = x.shape[0], x.shape[1], x.shape[2], w1.shape[0]
    d.e, d.w1, d.w2 = x.data_ptr(), w1.data_ptr(), w2.data_ptr()
    return d


class _SENetFn(torch.autograd.Function):
    """v [B, F, D] = x * a[:, :, None] of the SENet layer (csrc/fibinet.hip); w1 [R, F], w2 [F, R].  `saved` = a [B, F], then the
    hidden units [B, R]."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        lib = N.lib()
        x, w1, w2 = x.contiguous(), w1.contiguous(), w2.contiguous()
        d = _senet_desc(x, w1, w2)
        saved = torch.empty(_native_size(lib.satrans_senet_saved_floats, d), dtype=torch.float32, device=x.device)
        v = torch.empty_like(x)
        N.check(lib.satrans_senet_fwd(C.byref(d), v.data_ptr(), saved.data_ptr(), N.stream_handle(x.device)), "satrans_senet_fwd")
        ctx.save_for_backward(x, saved, w1, w2)
        ctx.mark_non_differentiable(saved)
        return v, saved

    @staticmethod
    def backward(ctx, dv, _dsaved):
        lib = N.lib()
        x, saved, w1, w2 = ctx.saved_tensors
        d = _senet_desc(x, w1, w2)
        work = torch.empty(_native_size(lib.satrans_senet_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.zeros_like(x)      # (the backward adds into it)
        dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
        g = N.SENetGrads()
        g.w1, g.w2 = dw1.data_ptr(), dw2.data_ptr()
        N.check(lib.satrans_senet_bwd(C.byref(d), None, dv.contiguous().data_ptr(), saved.data_ptr(), dx.data_ptr(), work.data_ptr(),
                                      C.byref(g), N.stream_handle(x.device)), "satrans_senet_bwd")
        return dx, dw1, dw2


class SENETLayer(nn.Module):
    """deepctr-torch's SENET layer, which the reference's FiBiNET calls (models/fibinet.py:51,93), with deepctr's constructor
    (its spelling `filed_size` included): `seed` and `device` are accepted and unused.  With inputs [B, F, D]:

        Z = mean(inputs, -1);  A = relu(relu(Z W1^T) W2^T);  V = inputs * A[:, :, None]

    forward(inputs [B, filed_size, D] fp32 on the GPU) -> [B, filed_size, D].  One autograd.Function runs satrans_senet_fwd /
    satrans_senet_bwd (csrc/fibinet.hip): a wave per row each way.  Parameters are deepctr's, `excitation.0.weight` [R, F] and
    `excitation.2.weight` [F, R], R = max(1, filed_size // reduction_ratio), with torch's Linear default initialisation in
    deepctr's order.  Not built - NotImplementedError: more than FIBINET_MAX_FIELDS fields (at construction), D beyond
    FIBINET_MAX_DIM (at the call)."""

    def __init__(self, filed_size, reduction_ratio=3, seed=1024, device='cpu'):
        super().__init__()
        filed_size = int(filed_size)
        if filed_size < 2 or reduction_ratio < 1:
            raise ValueError("SENETLayer: filed_size must be at least 2 and reduction_ratio at least 1")
        if filed_size > N.FIBINET_MAX_FIELDS:
            raise NotImplementedError(f"SENETLayer: up to FIBINET_MAX_FIELDS = {N.FIBINET_MAX_FIELDS} fields, got {filed_size}")
        self.seed = seed
        self.filed_size = filed_size
        self.reduction_size = max(1, filed_size // int(reduction_ratio))
        self.excitation = nn.Sequential(nn.Linear(self.filed_size, self.reduction_size, bias=False), nn.ReLU(),
                                        nn.Linear(self.reduction_size, self.filed_size, bias=False), nn.ReLU())

    def forward(self, inputs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        if inputs.shape[1] != self.filed_size:
            raise ValueError(f"SENETLayer: expected inputs [B, {self.filed_size}, D], got {tuple(inputs.shape)}")
        N.require_gpu(inputs, "SENETLayer")
        if inputs.dtype != torch.float32 or self.excitation[0].weight.dtype != torch.float32:
            raise TypeError("SENETLayer: inputs, parameters and gradients are float32")
        if inputs.shape[2] > N.FIBINET_MAX_DIM:
            raise NotImplementedError(f"SENETLayer: D up to FIBINET_MAX_DIM = {N.FIBINET_MAX_DIM}, got {inputs.shape[2]}")
        v, _ = _SENetFn.apply(inputs, self.excitation[0].weight, self.excitation[2].weight)
        return v


def _bilinear_desc(x, kind, w, a=None):
    d = N.BilinearDesc()
    d.B, d.F, d.D, d.type = x.shape[0], x.shape[1], x.shape[2], kind
    d.e, d.w, d.a = x.data_ptr(), w.data_ptr(), None if a is None else a.data_ptr()
    return d


class _BilinearFn(torch.autograd.Function):
    """out [B, P, D] of the bilinear interaction (csrc/fibinet.hip); `weights`: the Linear weights [D, D] in deepctr's order."""

    @staticmethod
    def forward(ctx, x, kind, *weights):
        lib = N.lib()
        x = x.contiguous()
        w = torch.stack(weights)
        F = x.shape[1]
        out = torch.empty(x.shape[0], F * (F - 1) // 2, x.shape[2], dtype=torch.float32, device=x.device)
        N.check(lib.satrans_bilinear_fwd(C.byref(_bilinear_desc(x, kind, w)), out.data_ptr(), N.stream_handle(x.device)),
                "satrans_bilinear_fwd")
        ctx.kind = kind
        ctx.save_for_backward(x, w, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = N.lib()
        x, w, out = ctx.saved_tensors
        d = _bilinear_desc(x, ctx.kind, w)
        work = torch.empty(_native_size(lib.satrans_bilinear_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        N.check(lib.satrans_bilinear_bwd(C.byref(d), dout.contiguous().data_ptr(), out.data_ptr(), dx.data_ptr(), None, work.data_ptr(),
                                         dw.data_ptr(), N.stream_handle(x.device)), "satrans_bilinear_bwd")
        return (dx, None, *dw.unbind(0))


def _bilinear_modules(filed_size, embedding_size, bilinear_type):
    """deepctr's `bilinear` attribute: one Linear ('all'), one per field ('each'), one per pair ('interaction')."""
    if bilinear_type == "all":
        return nn.Linear(embedding_size, embedding_size, bias=False)
    if bilinear_type == "each":
        return nn.ModuleList([nn.Linear(embedding_size, embedding_size, bias=False) for _ in range(filed_size)])
    if bilinear_type == "interaction":
        return nn.ModuleList([nn.Linear(embedding_size, embedding_size, bias=False)
                              for _ in range(filed_size * (filed_size - 1) // 2)])
    raise NotImplementedError


class BilinearInteraction(nn.Module):
    """deepctr-torch's bilinear interaction, which the reference's FiBiNET calls (models/fibinet.py:52,94-95), with deepctr's
    constructor: `seed` and `device` are accepted and unused.  For the pairs (i, j), i < j, in itertools.combinations order:

        'all'          bilinear(x_i) * x_j               one Linear(D, D, bias=False), `bilinear.weight`
        'each'         bilinear[i](x_i) * x_j            one per field, `bilinear.{i}.weight`; the last is never used and its
                                                         gradient is zero
        'interaction'  bilinear[p](x_i) * x_j            one per pair, `bilinear.{p}.weight`

    forward(inputs [B, filed_size, embedding_size] fp32 on the GPU) -> [B, P, embedding_size], P = F (F - 1) / 2.  One
    autograd.Function runs satrans_bilinear_fwd / satrans_bilinear_bwd (csrc/fibinet.hip): all pairs in one launch on the exact
    f32-input MFMA; the backward recomputes bilinear(x_i) instead of keeping it.  Parameters have deepctr's names, shapes,
    order and initialisation.  An unknown type raises NotImplementedError, as deepctr does; so do more than
    FIBINET_MAX_FIELDS fields and an embedding size beyond FIBINET_MAX_DIM."""

    def __init__(self, filed_size, embedding_size, bilinear_type="interaction", seed=1024, device='cpu'):
        super().__init__()
        filed_size, embedding_size = int(filed_size), int(embedding_size)
        if bilinear_type not in N.BILINEAR_TYPES:
            raise NotImplementedError
        if filed_size < 2 or embedding_size < 1:
            raise ValueError("BilinearInteraction: filed_size must be at least 2 and embedding_size positive")
        if filed_size > N.FIBINET_MAX_FIELDS:
            raise NotImplementedError(f"BilinearInteraction: up to FIBINET_MAX_FIELDS = {N.FIBINET_MAX_FIELDS} fields, got {filed_size}")
        if embedding_size > N.FIBINET_MAX_DIM:
            raise NotImplementedError(f"BilinearInteraction: embedding_size up to FIBINET_MAX_DIM = {N.FIBINET_MAX_DIM}, got "
                                      f"{embedding_size}")
        self.bilinear_type, self.seed = bilinear_type, seed
        self.filed_size, self.embedding_size = filed_size, embedding_size
        self.bilinear = _bilinear_modules(filed_size, embedding_size, bilinear_type)

    def weights(self):
        return [self.bilinear.weight] if self.bilinear_type == "all" else [m.weight for m in self.bilinear]

    def forward(self, inputs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        if inputs.shape[1] != self.filed_size or inputs.shape[2] != self.embedding_size:
            raise ValueError(f"BilinearInteraction: expected inputs [B, {self.filed_size}, {self.embedding_size}], got "
                             f"{tuple(inputs.shape)}")
        N.require_gpu(inputs, "BilinearInteraction")
        if inputs.dtype != torch.float32 or self.weights()[0].dtype != torch.float32:
            raise TypeError("BilinearInteraction: inputs, parameters and gradients are float32")
        return _BilinearFn.apply(inputs, N.BILINEAR_TYPES[self.bilinear_type], *self.weights())


def _fibinet_fill(tgt, n_dnn, se_w1, se_w2, bil_w, dnn, dnn_linear_w, out_bias):
    """Set the parameter pointers of a satrans_fibinet_desc / satrans_fibinet_grads; `dnn`: the weights, then the biases."""
    tgt.se_w1, tgt.se_w2, tgt.bilinear_w = se_w1.data_ptr(), se_w2.data_ptr(), bil_w.data_ptr()
    for l in range(n_dnn):
        tgt.dnn_w[l], tgt.dnn_b[l] = dnn[l].data_ptr(), dnn[n_dnn + l].data_ptr()
    tgt.dnn_linear_w, tgt.out_bias = dnn_linear_w.data_ptr(), out_bias.data_ptr()
    return tgt


def _fibinet_desc(emb, dense, kind, se_w1, se_w2, bil_w, dnn, dnn_linear_w, out_bias):
    n_dnn = len(dnn) // 2
    d = _fibinet_fill(N.FiBiNETDesc(), n_dnn, se_w1, se_w2, bil_w, dnn, dnn_linear_w, out_bias)
    d.B, d.F, d.D, d.type, d.R = emb.shape[0], emb.shape[1], emb.shape[2], kind, se_w1.shape[0]
    d.dense_dim, d.n_dnn = 0 if dense is None else dense.shape[1], n_dnn
    for l in range(n_dnn):
        d.width[l] = dnn[l].shape[0]
    d.emb, d.dense = emb.data_ptr(), None if dense is None else dense.data_ptr()
    return d


class _FiBiNETFn(torch.autograd.Function):
    """logit [B, 1] of the FiBiNET head (csrc/fibinet.hip).  `tensors`: se_w1, se_w2, the n_bil bilinear weights, the DNN's
    weights, its biases, dnn_linear's weight, out.bias.  `saved` = a, the hidden units, the DNN input, the DNN's hidden rows."""

    @staticmethod
    def forward(ctx, emb, dense, kind, n_bil, *tensors):
        lib = N.lib()
        dev = emb.device
        emb = emb.contiguous()
        dense = None if dense is None else dense.contiguous()
        se_w1, se_w2 = tensors[0].contiguous(), tensors[1].contiguous()
        bil_w = torch.stack(tensors[2:2 + n_bil])
        dnn = tuple(t.contiguous() for t in tensors[2 + n_bil:-2])
        dnn_linear_w, out_bias = tensors[-2].contiguous(), tensors[-1].contiguous()
        d = _fibinet_desc(emb, dense, kind, se_w1, se_w2, bil_w, dnn, dnn_linear_w, out_bias)
        saved = torch.empty(_native_size(lib.satrans_fibinet_saved_floats, d), dtype=torch.float32, device=dev)
        logit = torch.empty(emb.shape[0], 1, dtype=torch.float32, device=dev)
        N.check(lib.satrans_fibinet_fwd(C.byref(d), logit.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_fibinet_fwd")
        ctx.kind, ctx.has_dense = kind, dense is not None
        ctx.save_for_backward(emb, saved, se_w1, se_w2, bil_w, dnn_linear_w, out_bias, *dnn, *(() if dense is None else (dense,)))
        ctx.mark_non_differentiable(saved)
        return logit, saved

    @staticmethod
    def backward(ctx, dlogit, _dsaved):
        lib = N.lib()
        emb, saved, se_w1, se_w2, bil_w, dnn_linear_w, out_bias, *rest = ctx.saved_tensors
        dense = rest.pop() if ctx.has_dense else None
        dnn = tuple(rest)
        d = _fibinet_desc(emb, dense, ctx.kind, se_w1, se_w2, bil_w, dnn, dnn_linear_w, out_bias)
        work = torch.empty(_native_size(lib.satrans_fibinet_workspace_floats, d), dtype=torch.float32, device=emb.device)
        demb = torch.empty_like(emb)
        ddense = None if dense is None else torch.empty_like(dense)
        grads = [torch.empty_like(t) for t in (se_w1, se_w2, bil_w, *dnn, dnn_linear_w, out_bias)]
        g = _fibinet_fill(N.FiBiNETGrads(), len(dnn) // 2, grads[0], grads[1], grads[2], grads[3:-2], grads[-2], grads[-1])
        N.check(lib.satrans_fibinet_bwd(C.byref(d), dlogit.contiguous().data_ptr(), demb.data_ptr(),
                                        None if ddense is None else ddense.data_ptr(), saved.data_ptr(), work.data_ptr(), C.byref(g),
                                        N.stream_handle(emb.device)), "satrans_fibinet_bwd")
        return (demb, ddense, None, None, grads[0], grads[1], *grads[2].unbind(0), *grads[3:])


class FiBiNETHead(nn.Module):
    """The half of the reference's FiBiNET.forward behind the embedding lookup (models/fibinet.py:91-112):

        S = Bilinear(SE(emb));  R = Bilinear(emb);  dnn_input = cat(flatten(cat(S, R, dim=1)), dense)
        logit = linear_logit + dnn_linear(dnn(dnn_input)) + out.bias

    forward(emb [B, field_size, embedding_size] fp32, dense [B, dense_dim] or None, linear_logit [B,1] or None) -> logit [B,1];
    the caller applies the sigmoid.  `emb` is the concatenation of the looked-up embeddings of ALL sparse fields in field order,
    the domain column included; the reference's `metatrans` flag (fibinet.py:83-86) transforms that block first:

        head = FiBiNETHead(F, D, dense_dim, ...); meta = MetaTransformation(D, num_domains)
        logit = head(meta(domain_ids, emb), dense, linear_logit)

    The whole head is ONE autograd.Function over satrans_fibinet_fwd / satrans_fibinet_bwd (csrc/fibinet.hip): the excitation,
    both bilinear blocks from one D x D product per pair written straight into the DNN input, and the DNN itself - the widest of
    any baseline, [B, F (F - 1) D + dense_dim] - on the dense layer launcher of csrc/head_layers.h.  linear_logit is added
    outside it.  Empty dnn_hidden_units puts dnn_linear directly on the DNN input.

    Parameter names, shapes, state_dict order and initialisation are the reference FiBiNET's: out.bias (zeros),
    SE.excitation.{0,2}.weight, Bilinear.bilinear[.{i}].weight, dnn.linears.{l}.{weight,bias} (weights N(0, init_std)),
    dnn_linear.weight - those entries of a reference checkpoint load with load_state_dict.  An unused 'each' weight gets a
    zero gradient (the reference leaves it None).
    regularization_loss() -> [1] is what FiBiNET.__init__ itself adds to the reference's regularization_weight: nothing.
    The reference's fibinet.py has no add_regularization_weight call (the recorded runs pin that), so the result is zero;
    `l2_reg_linear` is accepted as the reference's constructor accepts it, where it reaches BaseModel's linear model only.
    Not built: dropout, batch-norm and activations other than relu in the DNN
    (NotImplementedError); bf16; more than MMOE_MAX_HIDDEN hidden layers, FIBINET_MAX_FIELDS fields, an embedding size beyond
    FIBINET_MAX_DIM (NotImplementedError at construction)."""

    def __init__(self, field_size, embedding_size, dense_dim=0, bilinear_type='interaction', reduction_ratio=3,
                 dnn_hidden_units=(128, 128), l2_reg_linear=1e-5, init_std=0.0001, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False):
        super().__init__()
        if bilinear_type not in N.BILINEAR_TYPES:
            raise NotImplementedError
        if field_size < 2:
            raise ValueError("FiBiNETHead: field_size must be at least 2 (one pair)")
        if embedding_size < 1 or dense_dim < 0 or reduction_ratio < 1:
            raise ValueError("FiBiNETHead: embedding_size must be positive, dense_dim non-negative, reduction_ratio at least 1")
        if dnn_dropout != 0 or dnn_use_bn or dnn_activation != 'relu':
            raise NotImplementedError("FiBiNETHead: dropout, batch-norm and activations other than relu are not built")
        units = [int(u) for u in dnn_hidden_units]
        if len(units) > N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"FiBiNETHead: up to MMOE_MAX_HIDDEN = {N.MMOE_MAX_HIDDEN} hidden layers, got {len(units)}")
        self.field_size, self.embedding_size, self.dense_dim = int(field_size), int(embedding_size), int(dense_dim)
        self.bilinear_type, self.l2_reg_linear = bilinear_type, float(l2_reg_linear)
        n = self.field_size * (self.field_size - 1) * self.embedding_size + self.dense_dim
        # (first: in the reference's state_dict `out.*` precedes FiBiNET's own modules, because its BaseModel registers that name)
        self.out = _OutBias()
        self.SE = SENETLayer(self.field_size, reduction_ratio)
        self.Bilinear = BilinearInteraction(self.field_size, self.embedding_size, bilinear_type)
        self.dnn = _TowerDNN(n, units, init_std)
        self.dnn_linear = nn.Linear(units[-1] if units else n, 1, bias=False)

    def regularization_loss(self):
        return torch.zeros((1,), device=self.dnn_linear.weight.device)

    def forward(self, emb, dense=None, linear_logit=None):
        if emb.dim() != 3 or emb.shape[1] != self.field_size or emb.shape[2] != self.embedding_size:
            raise ValueError(f"FiBiNETHead: expected emb [B, {self.field_size}, {self.embedding_size}], got {tuple(emb.shape)}")
        got = 0 if dense is None else (dense.shape[1] if dense.dim() == 2 else -1)
        if got != self.dense_dim:
            raise ValueError(f"FiBiNETHead: expected dense [B, {self.dense_dim}], got "
                             f"{None if dense is None else tuple(dense.shape)}")
        N.require_gpu(emb, "FiBiNETHead")
        if emb.dtype != torch.float32 or self.dnn_linear.weight.dtype != torch.float32:
            raise TypeError("FiBiNETHead: rows, parameters and gradients are float32")
        bil = self.Bilinear.weights()
        tensors = ([self.SE.excitation[0].weight, self.SE.excitation[2].weight] + bil + [lin.weight for lin in self.dnn.linears] +
                   [lin.bias for lin in self.dnn.linears] + [self.dnn_linear.weight, self.out.bias])
        logit, _ = _FiBiNETFn.apply(emb, dense if self.dense_dim else None, N.BILINEAR_TYPES[self.bilinear_type], len(bil), *tensors)
        return logit if linear_logit is None else linear_logit + logit


def _pieces(inputs, what, family="PNN"):
    """[B, F, D] of deepctr's list of [B, 1, D] pieces (or of a [B, F, D] tensor as it is); `family`: whose limits apply."""
    x = torch.cat(list(inputs), dim=1) if isinstance(inputs, (list, tuple)) else inputs
    if x.dim() != 3 or x.shape[1] < 2:
        raise ValueError(f"{what}: expected [B, F, D] with F >= 2 or a list of [B, 1, D] pieces, got {tuple(x.shape)}")
    N.require_gpu(x, what)
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: inputs, parameters and gradients are float32")
    max_fields, max_dim = getattr(N, f"{family}_MAX_FIELDS"), getattr(N, f"{family}_MAX_DIM")
    if x.shape[1] > max_fields or x.shape[2] > max_dim:
        raise NotImplementedError(f"{what}: up to {family}_MAX_FIELDS = {max_fields} fields and D up to {family}_MAX_DIM = "
                                  f"{max_dim}, got {tuple(x.shape)}")
    return x


def _inner_desc(x):
    d = N.InnerProductDesc()
    d.B, d.F, d.D, d.e = x.shape[0], x.shape[1], x.shape[2], x.data_ptr()
    return d


class _InnerProductFn(torch.autograd.Function):
    """out [B, P] = <x_i, x_j> over the pairs (csrc/pnn.hip)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        F = x.shape[1]
        out = torch.empty(x.shape[0], F * (F - 1) // 2, dtype=torch.float32, device=x.device)
        N.check(N.lib().satrans_inner_product_fwd(C.byref(_inner_desc(x)), out.data_ptr(), N.stream_handle(x.device)),
                "satrans_inner_product_fwd")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, = ctx.saved_tensors
        dx = torch.empty_like(x)
        N.check(N.lib().satrans_inner_product_bwd(C.byref(_inner_desc(x)), dout.contiguous().data_ptr(), dx.data_ptr(),
                                                  N.stream_handle(x.device)), "satrans_inner_product_bwd")
        return dx


class InnerProductLayer(nn.Module):
    """deepctr-torch's inner product layer, which the reference's PNN calls (models/pnn.py:61,95-96), with deepctr's constructor
    (`device` is accepted and unused).  For the pairs (i, j), i < j, in the order of deepctr's double loop:

        out[b, p, 0] = sum_d x_i[b, d] x_j[b, d]

    forward(inputs: [B, F, D] fp32 on the GPU, or deepctr's list of F pieces [B, 1, D]) -> [B, P, 1], P = F (F - 1) / 2, as
    deepctr returns it.  No parameters.  One autograd.Function runs satrans_inner_product_fwd / satrans_inner_product_bwd
    (csrc/pnn.hip): a workgroup reads a row once and writes all of its products; deepctr's two gathered [B, P, D] tensors are
    never formed.  Not built - NotImplementedError: reduce_sum=False (the [B, P, D] elementwise products, which PNN never
    uses), more than PNN_MAX_FIELDS fields, D beyond PNN_MAX_DIM."""

    def __init__(self, reduce_sum=True, device='cpu'):
        super().__init__()
        if not reduce_sum:
            raise NotImplementedError("InnerProductLayer: reduce_sum=False is not built (PNN does not use it)")
        self.reduce_sum = reduce_sum

    def forward(self, inputs):
        return _InnerProductFn.apply(_pieces(inputs, "InnerProductLayer")).unsqueeze(2)


def _outer_desc(x, kind, kernel):
    d = N.OuterProductDesc()
    d.B, d.F, d.D, d.kernel_type = x.shape[0], x.shape[1], x.shape[2], kind
    d.e, d.kernel = x.data_ptr(), kernel.data_ptr()
    return d


class _OuterProductFn(torch.autograd.Function):
    """out [B, P] of the outer product layer (csrc/pnn.hip); `kernel` in deepctr's shape of its type."""

    @staticmethod
    def forward(ctx, x, kind, kernel):
        x, kernel = x.contiguous(), kernel.contiguous()
        F = x.shape[1]
        out = torch.empty(x.shape[0], F * (F - 1) // 2, dtype=torch.float32, device=x.device)
        N.check(N.lib().satrans_outer_product_fwd(C.byref(_outer_desc(x, kind, kernel)), out.data_ptr(), N.stream_handle(x.device)),
                "satrans_outer_product_fwd")
        ctx.kind = kind
        ctx.save_for_backward(x, kernel)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = N.lib()
        x, kernel = ctx.saved_tensors
        d = _outer_desc(x, ctx.kind, kernel)
        work = torch.empty(_native_size(lib.satrans_outer_product_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx, dk = torch.empty_like(x), torch.empty_like(kernel)
        N.check(lib.satrans_outer_product_bwd(C.byref(d), dout.contiguous().data_ptr(), dx.data_ptr(), work.data_ptr(), dk.data_ptr(),
                                              N.stream_handle(x.device)), "satrans_outer_product_bwd")
        return dx, None, dk


def _outer_kernel(field_size, embedding_size, kernel_type):
    """deepctr's `kernel` parameter of a type, xavier-uniform as deepctr initialises it."""
    n_pairs = field_size * (field_size - 1) // 2
    shape = {"mat": (embedding_size, n_pairs, embedding_size), "vec": (n_pairs, embedding_size), "num": (n_pairs, 1)}[kernel_type]
    kernel = nn.Parameter(torch.empty(*shape))
    nn.init.xavier_uniform_(kernel)
    return kernel


class OutterProductLayer(nn.Module):
    """deepctr-torch's outer product layer under the reference's spelling, which its PNN calls (models/pnn.py:65,98-99), with
    deepctr's constructor (`seed` and `device` are accepted and unused).  With K_p = kernel[:, p, :]:

        'mat'   out[b, p] = x_j^T K_p x_i                       kernel [D, P, D]
        'vec'   out[b, p] = sum_d x_i[d] x_j[d] kernel[p, d]    kernel [P, D]
        'num'   out[b, p] = kernel[p, 0] sum_d x_i[d] x_j[d]    kernel [P, 1]

    forward(inputs: [B, field_size, embedding_size] fp32 on the GPU, or deepctr's list of pieces [B, 1, D]) -> [B, P].  One
    autograd.Function runs satrans_outer_product_fwd / satrans_outer_product_bwd (csrc/pnn.hip): 'mat' is one D x D product per
    pair on the exact f32-input MFMA with the kernel read in place, reduced to one float per row and pair inside the workgroup;
    deepctr's [B, D, P, D] product is never formed.  `kernel` has deepctr's shape and its xavier-uniform initial bits under a
    seed.  Another kernel_type raises the reference's ValueError; more than PNN_MAX_FIELDS fields or an embedding size beyond
    PNN_MAX_DIM NotImplementedError."""

    def __init__(self, field_size, embedding_size, kernel_type='mat', seed=1024, device='cpu'):
        super().__init__()
        if kernel_type not in N.PNN_KERNEL_TYPES:
            raise ValueError("kernel_type must be mat,vec or num")
        field_size, embedding_size = int(field_size), int(embedding_size)
        if field_size < 2 or embedding_size < 1:
            raise ValueError("OutterProductLayer: field_size must be at least 2 and embedding_size positive")
        if field_size > N.PNN_MAX_FIELDS:
            raise NotImplementedError(f"OutterProductLayer: up to PNN_MAX_FIELDS = {N.PNN_MAX_FIELDS} fields, got {field_size}")
        if embedding_size > N.PNN_MAX_DIM:
            raise NotImplementedError(f"OutterProductLayer: embedding_size up to PNN_MAX_DIM = {N.PNN_MAX_DIM}, got {embedding_size}")
        self.kernel_type, self.seed = kernel_type, seed
        self.field_size, self.embedding_size = field_size, embedding_size
        self.kernel = _outer_kernel(field_size, embedding_size, kernel_type)

    def forward(self, inputs):
        x = _pieces(inputs, "OutterProductLayer")
        if x.shape[1] != self.field_size or x.shape[2] != self.embedding_size:
            raise ValueError(f"OutterProductLayer: expected inputs [B, {self.field_size}, {self.embedding_size}], got {tuple(x.shape)}")
        if self.kernel.dtype != torch.float32:
            raise TypeError("OutterProductLayer: inputs, parameters and gradients are float32")
        return _OuterProductFn.apply(x, N.PNN_KERNEL_TYPES[self.kernel_type], self.kernel)


def _pnn_fill(tgt, n_dnn, kernel, dnn, dnn_linear_w, out_bias):
    """Set the parameter pointers of a satrans_pnn_desc / satrans_pnn_grads; `dnn`: the weights, then the biases."""
    tgt.kernel = None if kernel is None else kernel.data_ptr()
    for l in range(n_dnn):
        tgt.dnn_w[l], tgt.dnn_b[l] = dnn[l].data_ptr(), dnn[n_dnn + l].data_ptr()
    tgt.dnn_linear_w, tgt.out_bias = dnn_linear_w.data_ptr(), out_bias.data_ptr()
    return tgt


def _pnn_desc(emb, dense, cfg, kernel, dnn, dnn_linear_w, out_bias):
    n_dnn = len(dnn) // 2
    d = _pnn_fill(N.PNNDesc(), n_dnn, kernel, dnn, dnn_linear_w, out_bias)
    d.B, d.F, d.D = emb.shape
    d.use_inner, d.use_outer, d.kernel_type = cfg
    d.dense_dim, d.n_dnn = 0 if dense is None else dense.shape[1], n_dnn
    for l in range(n_dnn):
        d.width[l] = dnn[l].shape[0]
    d.emb, d.dense = emb.data_ptr(), None if dense is None else dense.data_ptr()
    return d


class _PNNFn(torch.autograd.Function):
    """logit [B, 1] of the PNN head (csrc/pnn.hip).  cfg = (use_inner, use_outer, kernel type); `tensors`: the outer product's
    kernel (with use_outer), the DNN's weights, its biases, dnn_linear's weight, out.bias.  `saved` = the DNN input, the DNN's
    hidden rows."""

    @staticmethod
    def forward(ctx, emb, dense, cfg, *tensors):
        lib = N.lib()
        dev = emb.device
        emb = emb.contiguous()
        dense = None if dense is None else dense.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        kernel = tensors[0] if cfg[1] else None
        dnn, dnn_linear_w, out_bias = tensors[(1 if cfg[1] else 0):-2], tensors[-2], tensors[-1]
        d = _pnn_desc(emb, dense, cfg, kernel, dnn, dnn_linear_w, out_bias)
        saved = torch.empty(_native_size(lib.satrans_pnn_saved_floats, d), dtype=torch.float32, device=dev)
        logit = torch.empty(emb.shape[0], 1, dtype=torch.float32, device=dev)
        N.check(lib.satrans_pnn_fwd(C.byref(d), logit.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_pnn_fwd")
        ctx.cfg, ctx.has_dense = cfg, dense is not None
        ctx.save_for_backward(emb, saved, *tensors, *(() if dense is None else (dense,)))
        ctx.mark_non_differentiable(saved)
        return logit, saved

    @staticmethod
    def backward(ctx, dlogit, _dsaved):
        lib = N.lib()
        emb, saved, *rest = ctx.saved_tensors
        dense = rest.pop() if ctx.has_dense else None
        kernel = rest[0] if ctx.cfg[1] else None
        dnn, dnn_linear_w, out_bias = tuple(rest[(1 if ctx.cfg[1] else 0):-2]), rest[-2], rest[-1]
        d = _pnn_desc(emb, dense, ctx.cfg, kernel, dnn, dnn_linear_w, out_bias)
        work = torch.empty(_native_size(lib.satrans_pnn_workspace_floats, d), dtype=torch.float32, device=emb.device)
        demb = torch.empty_like(emb)
        ddense = None if dense is None else torch.empty_like(dense)
        grads = [torch.empty_like(t) for t in rest]
        g = _pnn_fill(N.PNNGrads(), len(dnn) // 2, grads[0] if ctx.cfg[1] else None, grads[(1 if ctx.cfg[1] else 0):-2], grads[-2],
                      grads[-1])
        N.check(lib.satrans_pnn_bwd(C.byref(d), dlogit.contiguous().data_ptr(), demb.data_ptr(),
                                    None if ddense is None else ddense.data_ptr(), saved.data_ptr(), work.data_ptr(), C.byref(g),
                                    N.stream_handle(emb.device)), "satrans_pnn_bwd")
        return (demb, ddense, None, *grads)


class PNNHead(nn.Module):
    """The half of the reference's PNN.forward behind the embedding lookup (models/pnn.py:91-114):

        dnn_input = cat(flatten(emb), inner products (use_inner), outer products (use_outter), dense)
        logit = dnn_linear(dnn(dnn_input)) + out.bias

    forward(emb [B, field_size, embedding_size] fp32, dense [B, dense_dim] or None) -> logit [B,1]; the caller applies the
    sigmoid.  PNN has no linear model (pnn.py:43 passes no linear feature columns), so there is no linear_logit.  `emb` is the
    concatenation of the looked-up embeddings of ALL sparse fields in field order, the domain column included; the reference's
    `metatrans` flag (pnn.py:85-88) transforms that block first:

        head = PNNHead(F, D, dense_dim, ...); meta = MetaTransformation(D, num_domains)
        logit = head(meta(domain_ids, emb), dense)

    The whole head is ONE autograd.Function over satrans_pnn_fwd / satrans_pnn_bwd (csrc/pnn.hip): the products written
    straight into the DNN input (the 'mat' outer product one D x D product per pair on the matrix pipe, reduced inside the
    workgroup), the embedding gradient written once by one owner per element, and the DNN on the dense layer launcher of
    csrc/head_layers.h.  With neither product the head is the DNN over cat(flatten(emb), dense).  Empty dnn_hidden_units puts
    dnn_linear directly on the DNN input (the reference's constructor fails there).

    Parameter names, shapes, state_dict order and initialisation are the reference PNN's: out.bias (zeros),
    outterproduct.kernel (with use_outter; xavier-uniform), dnn.linears.{l}.{weight,bias} (weights N(0, init_std)),
    dnn_linear.weight - those entries of a reference checkpoint load with load_state_dict.
    regularization_loss() -> [1] is what PNN.__init__ itself adds to the reference's regularization_weight (pnn.py:74-76):
    l2_reg_dnn times the sum of squares of the DNN's weights (not biases) and of dnn_linear.weight, in
    get_regularization_loss's arithmetic.
    Not built: dropout and activations other than relu in the DNN (NotImplementedError);
    bf16; more than MMOE_MAX_HIDDEN hidden layers, PNN_MAX_FIELDS fields, an embedding size beyond PNN_MAX_DIM
    (NotImplementedError at construction)."""

    def __init__(self, field_size, embedding_size, dense_dim=0, dnn_hidden_units=(128, 128), use_inner=True, use_outter=False,
                 kernel_type='mat', l2_reg_dnn=0, init_std=0.0001, dnn_dropout=0, dnn_activation='relu'):
        super().__init__()
        if kernel_type not in N.PNN_KERNEL_TYPES:
            raise ValueError("kernel_type must be mat,vec or num")
        if field_size < 2:
            raise ValueError("PNNHead: field_size must be at least 2 (one pair)")
        if embedding_size < 1 or dense_dim < 0:
            raise ValueError("PNNHead: embedding_size must be positive, dense_dim non-negative")
        if dnn_dropout != 0 or dnn_activation != 'relu':
            raise NotImplementedError("PNNHead: dropout, batch-norm and activations other than relu are not built")
        units = [int(u) for u in dnn_hidden_units]
        if len(units) > N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"PNNHead: up to MMOE_MAX_HIDDEN = {N.MMOE_MAX_HIDDEN} hidden layers, got {len(units)}")
        if field_size > N.PNN_MAX_FIELDS:
            raise NotImplementedError(f"PNNHead: up to PNN_MAX_FIELDS = {N.PNN_MAX_FIELDS} fields, got {field_size}")
        if embedding_size > N.PNN_MAX_DIM:
            raise NotImplementedError(f"PNNHead: embedding_size up to PNN_MAX_DIM = {N.PNN_MAX_DIM}, got {embedding_size}")
        self.field_size, self.embedding_size, self.dense_dim = int(field_size), int(embedding_size), int(dense_dim)
        self.use_inner, self.use_outter, self.kernel_type = bool(use_inner), bool(use_outter), kernel_type
        self.l2_reg_dnn = float(l2_reg_dnn)
        n_pairs = self.field_size * (self.field_size - 1) // 2
        n = self.field_size * self.embedding_size + n_pairs * (int(self.use_inner) + int(self.use_outter)) + self.dense_dim
        # (first: in the reference's state_dict `out.*` precedes PNN's own modules, because its BaseModel registers that name)
        self.out = _OutBias()
        if self.use_inner:
            self.innerproduct = InnerProductLayer()
        if self.use_outter:
            self.outterproduct = OutterProductLayer(self.field_size, self.embedding_size, kernel_type)
        self.dnn = _TowerDNN(n, units, init_std)
        self.dnn_linear = nn.Linear(units[-1] if units else n, 1, bias=False)

    def regularization_loss(self):
        total = torch.zeros((1,), device=self.dnn_linear.weight.device)
        if self.l2_reg_dnn > 0:
            for p in [lin.weight for lin in self.dnn.linears] + [self.dnn_linear.weight]:
                total = total + torch.sum(self.l2_reg_dnn * torch.square(p))
        return total

    def forward(self, emb, dense=None):
        if emb.dim() != 3 or emb.shape[1] != self.field_size or emb.shape[2] != self.embedding_size:
            raise ValueError(f"PNNHead: expected emb [B, {self.field_size}, {self.embedding_size}], got {tuple(emb.shape)}")
        got = 0 if dense is None else (dense.shape[1] if dense.dim() == 2 else -1)
        if got != self.dense_dim:
            raise ValueError(f"PNNHead: expected dense [B, {self.dense_dim}], got {None if dense is None else tuple(dense.shape)}")
        N.require_gpu(emb, "PNNHead")
        if emb.dtype != torch.float32 or self.dnn_linear.weight.dtype != torch.float32:
            raise TypeError("PNNHead: rows, parameters and gradients are float32")
        tensors = (([self.outterproduct.kernel] if self.use_outter else []) + [lin.weight for lin in self.dnn.linears] +
                   [lin.bias for lin in self.dnn.linears] + [self.dnn_linear.weight, self.out.bias])
        cfg = (int(self.use_inner), int(self.use_outter), N.PNN_KERNEL_TYPES[self.kernel_type])
        logit, _ = _PNNFn.apply(emb, dense if self.dense_dim else None, cfg, *tensors)
        return logit


def _fm_desc(x):
    d = N.FMDesc()
    d.B, d.F, d.D, d.e = x.shape[0], x.shape[1], x.shape[2], x.data_ptr()
    return d


class _FMFn(torch.autograd.Function):
    """FM (pooled = False): out [B, 1]; BiInteractionPooling (pooled = True): out [B, 1, D] (csrc/fm.hip)."""

    @staticmethod
    def forward(ctx, x, pooled):
        x = x.contiguous()
        lib = N.lib()
        out = torch.empty((x.shape[0], 1, x.shape[2]) if pooled else (x.shape[0], 1), dtype=torch.float32, device=x.device)
        fn, name = (lib.satrans_bipool_fwd, "satrans_bipool_fwd") if pooled else (lib.satrans_fm_fwd, "satrans_fm_fwd")
        N.check(fn(C.byref(_fm_desc(x)), out.data_ptr(), N.stream_handle(x.device)), name)
        ctx.pooled = pooled
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, = ctx.saved_tensors
        lib = N.lib()
        dx = torch.empty_like(x)
        fn, name = (lib.satrans_bipool_bwd, "satrans_bipool_bwd") if ctx.pooled else (lib.satrans_fm_bwd, "satrans_fm_bwd")
        N.check(fn(C.byref(_fm_desc(x)), dout.contiguous().data_ptr(), dx.data_ptr(), N.stream_handle(x.device)), name)
        return dx, None


class FM(nn.Module):
    """deepctr-torch's factorization machine layer, which the reference's DeepFM and AFM call (models/deepfm.py:57,98,
    afm.py:51,71): the pairwise interactions without a linear term or a bias,

        out[b, 0] = 0.5 sum_d ((sum_f x_f[d])^2 - sum_f x_f[d]^2)

    forward(inputs: [B, F, D] fp32 on the GPU, or deepctr's list of F pieces [B, 1, D]) -> [B, 1].  No parameters.  One
    autograd.Function over satrans_fm_fwd / satrans_fm_bwd (csrc/fm.hip): one pass over the rows each way.  More than
    FM_MAX_FIELDS fields or D beyond FM_MAX_DIM: NotImplementedError."""

    def forward(self, inputs):
        return _FMFn.apply(_pieces(inputs, "FM", "FM"), False)


class BiInteractionPooling(nn.Module):
    """deepctr-torch's bi-interaction pooling, which the reference's NFM calls (models/nfm.py:56,75): FM's cross term before
    the sum over the embedding,

        out[b, 0, d] = 0.5 ((sum_f x_f[d])^2 - sum_f x_f[d]^2)

    forward(inputs: [B, F, D] fp32 on the GPU, or deepctr's list of pieces) -> [B, 1, D].  No parameters.  One autograd.Function
    over satrans_bipool_fwd / satrans_bipool_bwd (csrc/fm.hip).  Limits as FM's."""

    def forward(self, inputs):
        return _FMFn.apply(_pieces(inputs, "BiInteractionPooling", "FM"), True)


def _afm_fill(tgt, params, out_bias):
    for name, t in zip(N.AFM_POINTERS, params):
        setattr(tgt, name, t.data_ptr())
    tgt.out_bias = None if out_bias is None else out_bias.data_ptr()
    return tgt


def _afm_desc(x, params, linear_logit, out_bias):
    d = _afm_fill(N.AFMDesc(), params, out_bias)
    d.B, d.F, d.D = x.shape
    d.A = params[0].shape[1]
    d.e = x.data_ptr()
    d.linear_logit = None if linear_logit is None else linear_logit.data_ptr()
    return d


class _AFMFn(torch.autograd.Function):
    """out [B, 1] of AFMLayer, plus linear_logit and out.bias (each or None) in the same launch (csrc/fm.hip).  `saved` = the
    normalised attention scores [B, P], the attention output [B, D]."""

    @staticmethod
    def forward(ctx, x, linear_logit, out_bias, *params):
        lib = N.lib()
        x = x.contiguous()
        params = tuple(p.contiguous() for p in params)
        linear_logit = None if linear_logit is None else linear_logit.contiguous()
        d = _afm_desc(x, params, linear_logit, out_bias)
        saved = torch.empty(_native_size(lib.satrans_afm_saved_floats, d), dtype=torch.float32, device=x.device)
        out = torch.empty(x.shape[0], 1, dtype=torch.float32, device=x.device)
        N.check(lib.satrans_afm_fwd(C.byref(d), out.data_ptr(), saved.data_ptr(), N.stream_handle(x.device)), "satrans_afm_fwd")
        ctx.has_lin, ctx.has_bias = linear_logit is not None, out_bias is not None
        ctx.save_for_backward(x, saved, *params, *(() if out_bias is None else (out_bias,)))
        ctx.mark_non_differentiable(saved)
        return out, saved

    @staticmethod
    def backward(ctx, dout, _dsaved):
        lib = N.lib()
        x, saved, *params = ctx.saved_tensors
        out_bias = params.pop() if ctx.has_bias else None
        dout = dout.contiguous()
        d = _afm_desc(x, params, None, out_bias)
        work = torch.empty(_native_size(lib.satrans_afm_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(p) for p in params]
        dbias = None if out_bias is None else torch.empty_like(out_bias)
        g = _afm_fill(N.AFMGrads(), grads, dbias)
        N.check(lib.satrans_afm_bwd(C.byref(d), dout.data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(), C.byref(g),
                                    N.stream_handle(x.device)), "satrans_afm_bwd")
        return (dx, dout if ctx.has_lin else None, dbias, *grads)


class AFMLayer(nn.Module):
    """deepctr-torch's attentional factorization machine layer, which the reference's AFM calls (models/afm.py:47,69), with
    deepctr's constructor (`l2_reg_w`, `seed` and `device` are accepted and unused: the reference regularises attention_W through
    the model).  Over the pairs p = (i, j), i < j, in itertools.combinations order:

        x_p = x_i * x_j                                   a = softmax_p(relu(x_p attention_W + attention_b) projection_h)
        out = (sum_p a_p x_p) projection_p

    forward(inputs: deepctr's list of F pieces [B, 1, D], or [B, F, D], fp32 on the GPU) -> [B, 1].  Afterwards
    `normalized_att_score` [B, P, 1] holds the attention scores (detached), as deepctr's attribute does: it is the buffer the
    backward reads.  Parameters in deepctr's creation order: attention_W [D, A], attention_b [A] (zeros), projection_h [A, 1],
    projection_p [D, 1], the three matrices xavier-normal drawn in deepctr's order, so the initial bits under a seed are
    deepctr's.  One autograd.Function over satrans_afm_fwd / satrans_afm_bwd (csrc/fm.hip): a workgroup stages a sample's rows
    once and forms the pair products on chip; none of deepctr's [B, P, D] tensors exists, and the backward recomputes the
    products and the relu mask.  Not built - NotImplementedError: dropout_rate != 0; an attention factor beyond AFM_MAX_FACTOR;
    more than FM_MAX_FIELDS fields; an embedding size beyond FM_MAX_DIM."""

    def __init__(self, in_features, attention_factor=4, l2_reg_w=0, dropout_rate=0, seed=1024, device='cpu'):
        super().__init__()
        if dropout_rate != 0:
            raise NotImplementedError("AFMLayer: dropout is not built")
        in_features, attention_factor = int(in_features), int(attention_factor)
        if in_features < 1 or attention_factor < 1:
            raise ValueError("AFMLayer: in_features and attention_factor must be positive")
        if in_features > N.FM_MAX_DIM:
            raise NotImplementedError(f"AFMLayer: in_features up to FM_MAX_DIM = {N.FM_MAX_DIM}, got {in_features}")
        if attention_factor > N.AFM_MAX_FACTOR:
            raise NotImplementedError(f"AFMLayer: attention_factor up to AFM_MAX_FACTOR = {N.AFM_MAX_FACTOR}, got {attention_factor}")
        self.attention_factor, self.l2_reg_w, self.dropout_rate, self.seed = attention_factor, l2_reg_w, dropout_rate, seed
        self.attention_W = nn.Parameter(torch.empty(in_features, attention_factor))
        self.attention_b = nn.Parameter(torch.empty(attention_factor))
        self.projection_h = nn.Parameter(torch.empty(attention_factor, 1))
        self.projection_p = nn.Parameter(torch.empty(in_features, 1))
        for tensor in (self.attention_W, self.projection_h, self.projection_p):
            nn.init.xavier_normal_(tensor)
        nn.init.zeros_(self.attention_b)
        self.normalized_att_score = None

    def _run(self, inputs, linear_logit, out_bias, what):
        x = _pieces(inputs, what, "FM")
        if x.shape[2] != self.attention_W.shape[0]:
            raise ValueError(f"{what}: expected an embedding size of {self.attention_W.shape[0]}, got {tuple(x.shape)}")
        if self.attention_W.dtype != torch.float32:
            raise TypeError(f"{what}: inputs, parameters and gradients are float32")
        out, saved = _AFMFn.apply(x, linear_logit, out_bias, self.attention_W, self.attention_b, self.projection_h, self.projection_p)
        n_pairs = x.shape[1] * (x.shape[1] - 1) // 2
        self.normalized_att_score = saved[:x.shape[0] * n_pairs].view(x.shape[0], n_pairs, 1)
        return out

    def forward(self, inputs):
        return self._run(inputs, None, None, "AFMLayer")


def _fmhead_fill(tgt, n_dnn, dnn, dnn_linear_w, out_bias):
    """Set the parameter pointers of a satrans_fmhead_desc / satrans_fmhead_grads; `dnn`: the weights, then the biases."""
    for l in range(n_dnn):
        tgt.dnn_w[l], tgt.dnn_b[l] = dnn[l].data_ptr(), dnn[n_dnn + l].data_ptr()
    tgt.dnn_linear_w = None if dnn_linear_w is None else dnn_linear_w.data_ptr()
    tgt.out_bias = out_bias.data_ptr()
    return tgt


def _fmhead_desc(emb, dense, linear_logit, cfg, dnn, dnn_linear_w, out_bias):
    n_dnn = len(dnn) // 2
    d = _fmhead_fill(N.FMHeadDesc(), n_dnn, dnn, dnn_linear_w, out_bias)
    d.B, d.F, d.D = emb.shape
    d.kind, d.use_fm = cfg
    d.dense_dim, d.n_dnn = 0 if dense is None else dense.shape[1], n_dnn
    for l in range(n_dnn):
        d.width[l] = dnn[l].shape[0]
    d.emb, d.dense = emb.data_ptr(), None if dense is None else dense.data_ptr()
    d.linear_logit = None if linear_logit is None else linear_logit.data_ptr()
    return d


class _FMHeadFn(torch.autograd.Function):
    """logit [B, 1] of the DeepFM and NFM heads (csrc/fm.hip).  cfg = (kind, use_fm); `tensors`: the DNN's weights, its biases,
    dnn_linear's weight (those with a DNN), out.bias.  `saved` = the DNN input, the DNN's hidden rows."""

    @staticmethod
    def forward(ctx, emb, dense, linear_logit, cfg, *tensors):
        lib = N.lib()
        dev = emb.device
        emb = emb.contiguous()
        dense = None if dense is None else dense.contiguous()
        linear_logit = None if linear_logit is None else linear_logit.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        dnn, dnn_linear_w, out_bias = (tensors[:-2], tensors[-2], tensors[-1]) if len(tensors) > 1 else ((), None, tensors[-1])
        d = _fmhead_desc(emb, dense, linear_logit, cfg, dnn, dnn_linear_w, out_bias)
        saved = torch.empty(_native_size(lib.satrans_fmhead_saved_floats, d), dtype=torch.float32, device=dev)
        logit = torch.empty(emb.shape[0], 1, dtype=torch.float32, device=dev)
        N.check(lib.satrans_fmhead_fwd(C.byref(d), logit.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_fmhead_fwd")
        ctx.cfg, ctx.has_dense, ctx.has_lin = cfg, dense is not None, linear_logit is not None
        ctx.save_for_backward(emb, saved, *tensors, *(() if dense is None else (dense,)))
        ctx.mark_non_differentiable(saved)
        return logit, saved

    @staticmethod
    def backward(ctx, dlogit, _dsaved):
        lib = N.lib()
        emb, saved, *rest = ctx.saved_tensors
        dense = rest.pop() if ctx.has_dense else None
        dnn, dnn_linear_w, out_bias = (tuple(rest[:-2]), rest[-2], rest[-1]) if len(rest) > 1 else ((), None, rest[-1])
        dlogit = dlogit.contiguous()
        d = _fmhead_desc(emb, dense, None, ctx.cfg, dnn, dnn_linear_w, out_bias)
        work = torch.empty(_native_size(lib.satrans_fmhead_workspace_floats, d), dtype=torch.float32, device=emb.device)
        demb = torch.empty_like(emb)
        ddense = None if dense is None else torch.empty_like(dense)
        grads = [torch.empty_like(t) for t in rest]
        g = _fmhead_fill(N.FMHeadGrads(), len(dnn) // 2, grads[:-2], grads[-2] if dnn else None, grads[-1])
        N.check(lib.satrans_fmhead_bwd(C.byref(d), dlogit.data_ptr(), demb.data_ptr(), None if ddense is None else ddense.data_ptr(),
                                       saved.data_ptr(), work.data_ptr(), C.byref(g), N.stream_handle(emb.device)),
                "satrans_fmhead_bwd")
        return (demb, ddense, dlogit if ctx.has_lin else None, None, *grads)


class _FMFamilyHead(nn.Module):
    """What DeepFMHead and NFMHead share: the checks of a call, the DNN's parameters in the reference's order, the
    regularisation the reference's constructors register themselves."""

    def _init_dnn(self, what, n_in, dnn_hidden_units, l2_reg_dnn, init_std, refused):
        if refused:
            raise NotImplementedError(f"{what}: dropout, batch-norm and activations other than relu are not built")
        units = [int(u) for u in dnn_hidden_units]
        if len(units) > N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"{what}: up to MMOE_MAX_HIDDEN = {N.MMOE_MAX_HIDDEN} hidden layers, got {len(units)}")
        self.l2_reg_dnn = float(l2_reg_dnn)
        # (first: in the reference's state_dict `out.*` precedes the model's own modules, because its BaseModel registers that name)
        self.out = _OutBias()
        self.use_dnn = len(units) > 0
        if self.use_dnn:
            self.dnn = _TowerDNN(n_in, units, init_std)
            self.dnn_linear = nn.Linear(units[-1], 1, bias=False)

    @staticmethod
    def _check_sizes(what, field_size, embedding_size, dense_dim):
        if field_size is not None and field_size < 2:
            raise ValueError(f"{what}: field_size must be at least 2 (one pair)")
        if embedding_size < 1 or dense_dim < 0:
            raise ValueError(f"{what}: embedding_size must be positive, dense_dim non-negative")
        if field_size is not None and field_size > N.FM_MAX_FIELDS:
            raise NotImplementedError(f"{what}: up to FM_MAX_FIELDS = {N.FM_MAX_FIELDS} fields, got {field_size}")
        if embedding_size > N.FM_MAX_DIM:
            raise NotImplementedError(f"{what}: embedding_size up to FM_MAX_DIM = {N.FM_MAX_DIM}, got {embedding_size}")

    def regularization_loss(self):
        total = torch.zeros((1,), device=self.out.bias.device)
        if self.l2_reg_dnn > 0 and self.use_dnn:
            for p in [lin.weight for lin in self.dnn.linears] + [self.dnn_linear.weight]:
                total = total + torch.sum(self.l2_reg_dnn * torch.square(p))
        return total

    def _run(self, what, emb, dense, linear_logit, cfg):
        if emb.dim() != 3 or emb.shape[2] != self.embedding_size or emb.shape[1] < 2 or \
                (self.field_size is not None and emb.shape[1] != self.field_size):
            raise ValueError(f"{what}: expected emb [B, {self.field_size or 'F >= 2'}, {self.embedding_size}], got {tuple(emb.shape)}")
        got = 0 if dense is None else (dense.shape[1] if dense.dim() == 2 else -1)
        if got != self.dense_dim:
            raise ValueError(f"{what}: expected dense [B, {self.dense_dim}], got {None if dense is None else tuple(dense.shape)}")
        if linear_logit is not None and tuple(linear_logit.shape) != (emb.shape[0], 1):
            raise ValueError(f"{what}: expected linear_logit [B, 1], got {tuple(linear_logit.shape)}")
        N.require_gpu(emb, what)
        if emb.dtype != torch.float32 or self.out.bias.dtype != torch.float32:
            raise TypeError(f"{what}: rows, parameters and gradients are float32")
        if emb.shape[1] > N.FM_MAX_FIELDS:
            raise NotImplementedError(f"{what}: up to FM_MAX_FIELDS = {N.FM_MAX_FIELDS} fields, got {emb.shape[1]}")
        tensors = [self.out.bias]
        if self.use_dnn:
            tensors = ([lin.weight for lin in self.dnn.linears] + [lin.bias for lin in self.dnn.linears] +
                       [self.dnn_linear.weight, self.out.bias])
        logit, _ = _FMHeadFn.apply(emb, dense if self.dense_dim and self.use_dnn else None, linear_logit, cfg, *tensors)
        return logit


class DeepFMHead(_FMFamilyHead):
    """The half of the reference's DeepFM.forward behind the embedding lookup (models/deepfm.py:87-113):

        logit = linear_logit + FM(emb) (use_fm) + dnn_linear(dnn(cat(flatten(emb), dense))) (hidden units non-empty) + out.bias

    forward(emb [B, field_size, embedding_size] fp32, dense [B, dense_dim] or None, linear_logit [B, 1] or None) -> logit
    [B, 1]; the caller applies the sigmoid.  `linear_logit` is the port's own linear_model(X), as in XDeepFMHead; its gradient is
    the logit's.  use_fm=False serves the reference's `nofm` flag; empty dnn_hidden_units its `nodnn` flag, and then there are no
    dnn.* entries (and the dense values are not read); both off: ValueError.  The reference's `metatrans` flag transforms the
    embedding block first:

        head = DeepFMHead(F, D, dense_dim, ...); meta = MetaTransformation(D, num_domains)
        logit = head(meta(domain_ids, emb), dense, linear_logit)

    The whole head is ONE autograd.Function over satrans_fmhead_fwd / satrans_fmhead_bwd (csrc/fm.hip): one pass over the rows
    writes the FM term and linear_logit into the logit and the rows into the DNN input, the DNN runs on the dense layer launcher
    of csrc/head_layers.h and adds its column, and the embedding gradient is written once, the DNN input gradient's block plus
    the FM term.  Parameter names, state_dict order and initialisation are the reference DeepFM's: out.bias (zeros),
    dnn.linears.{l}.{weight,bias} (weights N(0, init_std)), dnn_linear.weight.  regularization_loss() -> [1] is what
    DeepFM.__init__ itself registers (deepfm.py:66-68): l2_reg_dnn times the squares of the DNN's weights and of
    dnn_linear.weight, in get_regularization_loss's arithmetic.
    Not built: a DeepFM model class behind BaseModel; dropout, batch-norm and activations other than relu (NotImplementedError);
    bf16; more than MMOE_MAX_HIDDEN hidden layers, FM_MAX_FIELDS fields, an embedding size beyond FM_MAX_DIM."""

    def __init__(self, field_size, embedding_size, dense_dim=0, use_fm=True, dnn_hidden_units=(256, 128), l2_reg_dnn=0,
                 init_std=0.0001, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False):
        super().__init__()
        self._check_sizes("DeepFMHead", field_size, embedding_size, dense_dim)
        if not use_fm and len(dnn_hidden_units) == 0:
            raise ValueError("DeepFMHead: neither the FM term nor a DNN")
        self.field_size, self.embedding_size, self.dense_dim = int(field_size), int(embedding_size), int(dense_dim)
        self.use_fm = bool(use_fm)
        self._init_dnn("DeepFMHead", self.field_size * self.embedding_size + self.dense_dim, dnn_hidden_units, l2_reg_dnn, init_std,
                       dnn_dropout != 0 or dnn_activation != 'relu' or dnn_use_bn)
        if self.use_fm:
            self.fm = FM()

    def forward(self, emb, dense=None, linear_logit=None):
        return self._run("DeepFMHead", emb, dense, linear_logit, (N.FMHEAD_DEEPFM, int(self.use_fm)))


class NFMHead(_FMFamilyHead):
    """The half of the reference's NFM.forward behind the embedding lookup (models/nfm.py:73-83):

        logit = linear_logit + dnn_linear(dnn(cat(BiInteractionPooling(emb)[:, 0, :], dense))) + out.bias

    forward(emb [B, F, embedding_size] fp32 (any 2 <= F <= FM_MAX_FIELDS), dense [B, dense_dim] or None, linear_logit [B, 1] or
    None) -> logit [B, 1]; the caller applies the sigmoid.  With the reference's `metatrans` flag:

        head = NFMHead(D, dense_dim, ...); meta = MetaTransformation(D, num_domains)
        logit = head(meta(domain_ids, emb), dense, linear_logit)

    ONE autograd.Function over satrans_fmhead_fwd / satrans_fmhead_bwd (csrc/fm.hip): the pooled row goes straight into the DNN
    input, the DNN runs on the dense layer launcher of csrc/head_layers.h, and the embedding gradient is written once from the
    DNN input gradient.  Parameter names, state_dict order and initialisation are the reference NFM's: out.bias,
    dnn.linears.{l}.{weight,bias}, dnn_linear.weight; regularization_loss() is what NFM.__init__ registers (nfm.py:53-55).
    Not built: bi_dropout, dnn_dropout, activations other than relu (NotImplementedError); empty dnn_hidden_units (ValueError:
    the reference's constructor fails there too); bf16; the limits of DeepFMHead."""

    def __init__(self, embedding_size, dense_dim=0, dnn_hidden_units=(128, 128), l2_reg_dnn=0, init_std=0.0001, bi_dropout=0,
                 dnn_dropout=0, dnn_activation='relu'):
        super().__init__()
        self._check_sizes("NFMHead", None, embedding_size, dense_dim)
        if len(dnn_hidden_units) == 0:
            raise ValueError("NFMHead: dnn_hidden_units must not be empty")
        self.field_size, self.embedding_size, self.dense_dim = None, int(embedding_size), int(dense_dim)
        self._init_dnn("NFMHead", self.embedding_size + self.dense_dim, dnn_hidden_units, l2_reg_dnn, init_std,
                       bi_dropout != 0 or dnn_dropout != 0 or dnn_activation != 'relu')
        self.bi_pooling = BiInteractionPooling()

    def forward(self, emb, dense=None, linear_logit=None):
        return self._run("NFMHead", emb, dense, linear_logit, (N.FMHEAD_NFM, 0))


class AFMHead(nn.Module):
    """The half of the reference's AFM.forward behind the embedding lookup (models/afm.py:66-73) with use_attention=True:

        logit = linear_logit + fm(emb) + out.bias,   fm = AFMLayer(embedding_size, attention_factor)

    forward(emb [B, F, embedding_size] fp32 or deepctr's list of pieces, linear_logit [B, 1] or None) -> logit [B, 1]; the
    caller applies the sigmoid.  linear_logit and out.bias enter in the AFM forward's epilogue, so the head is the same two
    launches as the layer; `fm.normalized_att_score` is set as by the layer.  With the reference's `metatrans` flag:

        head = AFMHead(D, ...); meta = MetaTransformation(D, num_domains)
        logit = head(meta(domain_ids, emb), linear_logit)

    state_dict keys in the reference's order: out.bias, fm.attention_W, fm.attention_b, fm.projection_h, fm.projection_p.
    regularization_loss() -> [1] is what AFM.__init__ registers (afm.py:49): l2_reg_att times the sum of squares of
    fm.attention_W.  use_attention=False is DeepFMHead(field_size, embedding_size, use_fm=True, dnn_hidden_units=()).
    Not built: afm_dropout (NotImplementedError); the limits of AFMLayer."""

    def __init__(self, embedding_size, attention_factor=8, l2_reg_att=1e-5, afm_dropout=0):
        super().__init__()
        if afm_dropout != 0:
            raise NotImplementedError("AFMHead: dropout is not built")
        self.embedding_size, self.l2_reg_att = int(embedding_size), float(l2_reg_att)
        # (first: in the reference's state_dict `out.*` precedes AFM's own modules, because its BaseModel registers that name)
        self.out = _OutBias()
        self.fm = AFMLayer(self.embedding_size, attention_factor, l2_reg_att, afm_dropout)

    def regularization_loss(self):
        total = torch.zeros((1,), device=self.out.bias.device)
        if self.l2_reg_att > 0:
            total = total + torch.sum(self.l2_reg_att * torch.square(self.fm.attention_W))
        return total

    def forward(self, emb, linear_logit=None):
        if linear_logit is not None and (linear_logit.dim() != 2 or linear_logit.shape[1] != 1):
            raise ValueError(f"AFMHead: expected linear_logit [B, 1], got {tuple(linear_logit.shape)}")
        return self.fm._run(emb, linear_logit, self.out.bias, "AFMHead")


def _interacting_flags(use_res, scaling):
    return (0 if use_res else N.NO_RES) | (0 if scaling else NO_SCALING)


def _interacting_desc(x, head_num, flags, weights):
    d = N.InteractingDesc()
    d.B, d.F, d.D = x.shape
    d.H, d.flags, d.x = head_num, flags, x.data_ptr()
    for name, w in zip(N.INTERACTING_POINTERS, weights):
        setattr(d, name, w.data_ptr())
    return d


class _InteractingFn(torch.autograd.Function):
    """y [B, F, D] of one InteractingLayer (csrc/autoint.hip).  cfg = (head_num, flags, capture); `weights`: W_Query, W_key,
    W_Value (, W_Res).  `saved` = the softmax rows' (max, sum), 2 B H F floats; `att` = the normalised scores [H, B, F, F]
    (empty unless capture)."""

    @staticmethod
    def forward(ctx, x, cfg, *weights):
        lib = N.lib()
        head_num, flags, capture = cfg
        x = x.contiguous()
        weights = tuple(w.contiguous() for w in weights)
        d = _interacting_desc(x, head_num, flags, weights)
        n = int(lib.satrans_interacting_saved_floats(C.byref(d)))
        if n < 0:
            raise N.NativeError(f"InteractingLayer: shape B={d.B} F={d.F} D={d.D} H={head_num} is not supported")
        saved = torch.empty(n, dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        att = torch.empty((head_num, d.B, d.F, d.F) if capture else (0,), dtype=torch.float32, device=x.device)
        N.check(lib.satrans_interacting_fwd(C.byref(d), y.data_ptr(), att.data_ptr() if capture else None, saved.data_ptr(),
                                            N.stream_handle(x.device)), "satrans_interacting_fwd")
        ctx.cfg = cfg
        ctx.save_for_backward(x, y, saved, *weights)
        ctx.mark_non_differentiable(saved, att)
        return y, saved, att

    @staticmethod
    def backward(ctx, dy, _dsaved, _datt):
        lib = N.lib()
        x, y, saved, *weights = ctx.saved_tensors
        d = _interacting_desc(x, ctx.cfg[0], ctx.cfg[1], weights)
        scratch = torch.empty(_native_size(lib.satrans_interacting_scratch_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        g = torch.empty(len(weights), d.D, d.D, dtype=torch.float32, device=x.device)
        N.check(lib.satrans_interacting_bwd(C.byref(d), y.data_ptr(), dy.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(),
                                            scratch.data_ptr(), g.data_ptr(), N.stream_handle(x.device)), "satrans_interacting_bwd")
        return (dx, None, *g.unbind(0))


class InteractingLayer(nn.Module):
    """deepctr-torch 0.2.9's InteractingLayer, the layer the reference's AutoInt stacks (models/autoint.py:13,75-76), with
    deepctr's constructor, its two ValueErrors, its parameter names (`W_key` has a lower-case k) and creation order - W_Query,
    W_key, W_Value, W_Res (with use_res) - every one drawn N(0, 0.05):

        q, k, v = x W_Query, x W_key, x W_Value;   per head h of D / head_num columns:  p = softmax_j(q_i . k_j), divided by
        sqrt(D / head_num) first with scaling (deepctr's default: off);   y = relu(p v + x W_Res)   (no residual: relu(p v))

    It is not SelfAttention_Layer (the reference's submodules.py:178-238): no W_Out, no dropout, no LayerNorm, `scaling`
    defaults to False, and a checkpoint of one does not load into the other.
    forward(inputs [B, F, D] fp32 on the GPU) -> [B, F, D]: ONE autograd.Function, one launch forward (satrans_interacting_fwd,
    csrc/autoint.hip), one launch plus an ordered reduce backward.  Only the softmax rows' (max, sum) are saved: 2 B H F floats;
    the backward recomputes q, k, v from the input and takes the relu mask from the output.
    `capture_attention` (default False) makes the forward also write `normalized_att_scores` [H, B, F, F], the switch
    SelfAttention_Layer has; deepctr fills that attribute on every forward, here it stays None until the switch is on.
    Shapes: D in {16, 32, 64}, D / head_num in {8, 16, 32}, 2 <= F <= 64; anything else raises NativeError at the call."""

    def __init__(self, embedding_size, head_num=2, use_res=True, scaling=False, seed=1024, device='cpu'):
        super().__init__()
        if head_num <= 0:
            raise ValueError('head_num must be a int > 0')
        if embedding_size % head_num != 0:
            raise ValueError('embedding_size is not an integer multiple of head_num!')
        self.att_embedding_size = embedding_size // head_num
        self.head_num, self.use_res, self.scaling, self.seed = head_num, use_res, scaling, seed
        self.W_Query = nn.Parameter(torch.Tensor(embedding_size, embedding_size))
        self.W_key = nn.Parameter(torch.Tensor(embedding_size, embedding_size))
        self.W_Value = nn.Parameter(torch.Tensor(embedding_size, embedding_size))
        if self.use_res:
            self.W_Res = nn.Parameter(torch.Tensor(embedding_size, embedding_size))
        for tensor in self.parameters():
            nn.init.normal_(tensor, mean=0.0, std=0.05)
        self.normalized_att_scores = None
        self.capture_attention = False
        self.to(device)

    def weights(self):
        return [self.W_Query, self.W_key, self.W_Value] + ([self.W_Res] if self.use_res else [])

    def forward(self, inputs):
        if len(inputs.shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(inputs.shape)))
        if inputs.shape[2] != self.W_Query.shape[0]:
            raise ValueError(f"InteractingLayer: expected an embedding size of {self.W_Query.shape[0]}, got {tuple(inputs.shape)}")
        N.require_gpu(inputs, "InteractingLayer")
        if inputs.dtype != torch.float32 or self.W_Query.dtype != torch.float32:
            raise TypeError("InteractingLayer: inputs, parameters and gradients are float32")
        cfg = (self.head_num, _interacting_flags(self.use_res, self.scaling), bool(self.capture_attention))
        y, _, att = _InteractingFn.apply(inputs, cfg, *self.weights())
        if self.capture_attention:
            self.normalized_att_scores = att
        return y


def _autoint_fill(tgt, n_dnn, dnn, dnn_linear_w, out_bias):
    """Set the DNN pointers of a satrans_autoint_desc / satrans_autoint_grads; `dnn`: the weights, then the biases."""
    for l in range(n_dnn):
        tgt.dnn_w[l], tgt.dnn_b[l] = dnn[l].data_ptr(), dnn[n_dnn + l].data_ptr()
    tgt.dnn_linear_w, tgt.out_bias = dnn_linear_w.data_ptr(), out_bias.data_ptr()
    return tgt


def _autoint_desc(emb, dense, cfg, int_w, dnn, dnn_linear_w, out_bias):
    head_num, flags, n_layers = cfg[:3]
    n_dnn = len(dnn) // 2
    d = _autoint_fill(N.AutoIntDesc(), n_dnn, dnn, dnn_linear_w, out_bias)
    d.B, d.F, d.D = emb.shape
    d.H, d.flags, d.n_layers = head_num, flags, n_layers
    d.dense_dim, d.n_dnn = 0 if dense is None else dense.shape[1], n_dnn
    for l in range(n_dnn):
        d.width[l] = dnn[l].shape[0]
    d.emb, d.dense = emb.data_ptr(), None if dense is None else dense.data_ptr()
    per = len(int_w) // n_layers
    for l in range(min(n_layers, N.AUTOINT_MAX_LAYERS)):
        for name, w in zip(N.INTERACTING_POINTERS, int_w[l * per:(l + 1) * per]):
            getattr(d, name)[l] = w.data_ptr()
    return d


class _AutoIntFn(torch.autograd.Function):
    """logit [B, 1] of the AutoInt head (csrc/autoint.hip).  cfg = (head_num, flags, n_layers, capture: a tuple of bools);
    `tensors`: the layers' weights layer by layer, the DNN's weights, its biases, dnn_linear's weight, out.bias.  `saved` = the
    layers' outputs, their softmax statistics, the DNN input, the DNN's hidden rows; `atts`: a captured layer's scores."""

    @staticmethod
    def forward(ctx, emb, dense, cfg, *tensors):
        lib = N.lib()
        dev = emb.device
        head_num, flags, n_layers, capture = cfg
        emb = emb.contiguous()
        dense = None if dense is None else dense.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        n_int = n_layers * (3 if flags & N.NO_RES else 4)
        int_w, dnn, dnn_linear_w, out_bias = tensors[:n_int], tensors[n_int:-2], tensors[-2], tensors[-1]
        d = _autoint_desc(emb, dense, cfg, int_w, dnn, dnn_linear_w, out_bias)
        n = int(lib.satrans_autoint_saved_floats(C.byref(d)))
        if n < 0:
            raise N.NativeError(f"AutoIntHead: shape B={d.B} F={d.F} D={d.D} H={head_num} with {n_layers} layers is not supported: "
                                f"{(lib.satrans_last_error() or b'').decode()}")
        saved = torch.empty(n, dtype=torch.float32, device=dev)
        logit = torch.empty(emb.shape[0], 1, dtype=torch.float32, device=dev)
        atts = [torch.empty((head_num, d.B, d.F, d.F) if on else (0,), dtype=torch.float32, device=dev) for on in capture]
        ptrs = (C.c_void_p * n_layers)(*[a.data_ptr() if on else None for a, on in zip(atts, capture)])
        N.check(lib.satrans_autoint_fwd(C.byref(d), logit.data_ptr(), ptrs, saved.data_ptr(), N.stream_handle(dev)), "satrans_autoint_fwd")
        ctx.cfg, ctx.has_dense, ctx.n_int = cfg, dense is not None, n_int
        ctx.save_for_backward(emb, saved, *tensors, *(() if dense is None else (dense,)))
        ctx.mark_non_differentiable(saved, *atts)
        return (logit, saved, *atts)

    @staticmethod
    def backward(ctx, dlogit, *_):
        lib = N.lib()
        emb, saved, *rest = ctx.saved_tensors
        dense = rest.pop() if ctx.has_dense else None
        n_int, n_layers = ctx.n_int, ctx.cfg[2]
        int_w, dnn, dnn_linear_w, out_bias = rest[:n_int], tuple(rest[n_int:-2]), rest[-2], rest[-1]
        d = _autoint_desc(emb, dense, ctx.cfg, int_w, dnn, dnn_linear_w, out_bias)
        work = torch.empty(_native_size(lib.satrans_autoint_workspace_floats, d), dtype=torch.float32, device=emb.device)
        demb = torch.empty_like(emb)
        ddense = None if dense is None else torch.empty_like(dense)
        per = n_int // n_layers
        g_int = torch.empty(n_layers, per, d.D, d.D, dtype=torch.float32, device=emb.device)
        grads = [torch.empty_like(t) for t in rest[n_int:]]
        g = _autoint_fill(N.AutoIntGrads(), len(dnn) // 2, grads[:-2], grads[-2], grads[-1])
        for l in range(n_layers):
            g.int_w[l] = g_int[l].data_ptr()
        N.check(lib.satrans_autoint_bwd(C.byref(d), dlogit.contiguous().data_ptr(), demb.data_ptr(),
                                        None if ddense is None else ddense.data_ptr(), saved.data_ptr(), work.data_ptr(), C.byref(g),
                                        N.stream_handle(emb.device)), "satrans_autoint_bwd")
        return (demb, ddense, None, *g_int.view(n_int, d.D, d.D).unbind(0), *grads)


class AutoIntHead(nn.Module):
    """The half of the reference's AutoInt.forward behind the embedding lookup (models/autoint.py:93-121):

        att_output = flatten(int_layers[L-1](... int_layers[0](emb)))
        logit = dnn_linear(cat(att_output, dnn(cat(flatten(emb), dense)))) + out.bias     (dnn_hidden_units non-empty)
        logit = dnn_linear(att_output) + out.bias                                         (dnn_hidden_units=())

    forward(emb [B, field_num, embedding_size] fp32 on the GPU, dense [B, dense_dim] or None) -> logit [B, 1]; the caller
    applies the sigmoid.  The reference's `logit = 0` holds: its linear model is not added (autoint.py:89-90), so there is no
    linear_logit argument.  `emb` is the concatenation of the looked-up embeddings of all sparse fields in field order, the
    domain column included; the reference's `usemetatrans` flag (autoint.py:84-87) transforms that block first and stays the
    caller's:

        head = AutoIntHead(F, D, dense_dim, ...); meta = MetaTransformation(D, num_domains)
        logit = head(meta(domain_ids, emb), dense)

    The whole head is ONE autograd.Function over satrans_autoint_fwd / satrans_autoint_bwd (csrc/autoint.hip): one launch per
    interacting layer each way plus the ordered reduce of its weight gradients, the DNN and both column blocks of dnn_linear on
    the dense layer launcher of csrc/head_layers.h, and the embedding gradient written once by the first layer's backward with
    the DNN input gradient added in its epilogue.  `int_layers` are InteractingLayer modules (deepctr's defaults: scaling off), so
    a layer can be driven alone, and a layer's `capture_attention` makes the head fill its `normalized_att_scores`.
    state_dict keys and their order are the reference's: out.bias (zeros), dnn_linear.weight (torch's default draw, bias-free),
    dnn.linears.{l}.{weight,bias} (weights N(0, init_std)), int_layers.{i}.W_Query / W_key / W_Value / W_Res.
    att_layer_num < 1: ValueError.  Not built: dropout, batch-norm and activations
    other than relu in the DNN (NotImplementedError); l2_reg_dnn; bf16; more than AUTOINT_MAX_LAYERS interacting or
    MMOE_MAX_HIDDEN hidden layers (NotImplementedError); shapes outside InteractingLayer's raise NativeError at the call."""

    def __init__(self, field_num, embedding_size, dense_dim=0, att_layer_num=3, att_head_num=2, att_res=True,
                 dnn_hidden_units=(256, 128), init_std=0.0001, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False):
        super().__init__()
        if att_layer_num < 1:
            raise ValueError("AutoIntHead: att_layer_num must be at least 1")
        if field_num < 2 or embedding_size < 1 or dense_dim < 0:
            raise ValueError("AutoIntHead: field_num must be at least 2, embedding_size positive, dense_dim non-negative")
        if dnn_dropout != 0 or dnn_use_bn or dnn_activation != 'relu':
            raise NotImplementedError("AutoIntHead: dropout, batch-norm and activations other than relu are not built")
        units = [int(u) for u in dnn_hidden_units]
        if len(units) > N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"AutoIntHead: up to MMOE_MAX_HIDDEN = {N.MMOE_MAX_HIDDEN} hidden layers, got {len(units)}")
        if att_layer_num > N.AUTOINT_MAX_LAYERS:
            raise NotImplementedError(f"AutoIntHead: up to AUTOINT_MAX_LAYERS = {N.AUTOINT_MAX_LAYERS} interacting layers, "
                                      f"got {att_layer_num}")
        self.field_num, self.embedding_size, self.dense_dim = int(field_num), int(embedding_size), int(dense_dim)
        self.att_layer_num, self.att_head_num, self.att_res = int(att_layer_num), int(att_head_num), bool(att_res)
        n_att = self.field_num * self.embedding_size
        # (first: in the reference's state_dict `out.*` precedes AutoInt's own modules, because its BaseModel registers that name;
        # dnn_linear before dnn: autoint.py:66-70)
        self.out = _OutBias()
        self.dnn_linear = nn.Linear(n_att + (units[-1] if units else 0), 1, bias=False)
        self.use_dnn = len(units) > 0
        if self.use_dnn:
            self.dnn = _TowerDNN(n_att + self.dense_dim, units, init_std)
        self.int_layers = nn.ModuleList([InteractingLayer(self.embedding_size, self.att_head_num, self.att_res)
                                         for _ in range(self.att_layer_num)])

    def forward(self, emb, dense=None):
        if emb.dim() != 3 or emb.shape[1] != self.field_num or emb.shape[2] != self.embedding_size:
            raise ValueError(f"AutoIntHead: expected emb [B, {self.field_num}, {self.embedding_size}], got {tuple(emb.shape)}")
        got = 0 if dense is None else (dense.shape[1] if dense.dim() == 2 else -1)
        if got != self.dense_dim:
            raise ValueError(f"AutoIntHead: expected dense [B, {self.dense_dim}], got {None if dense is None else tuple(dense.shape)}")
        N.require_gpu(emb, "AutoIntHead")
        if emb.dtype != torch.float32 or self.dnn_linear.weight.dtype != torch.float32:
            raise TypeError("AutoIntHead: rows, parameters and gradients are float32")
        capture = tuple(bool(layer.capture_attention) for layer in self.int_layers)
        cfg = (self.att_head_num, _interacting_flags(self.att_res, self.int_layers[0].scaling), self.att_layer_num, capture)
        tensors = [w for layer in self.int_layers for w in layer.weights()]
        if self.use_dnn:
            tensors += [lin.weight for lin in self.dnn.linears] + [lin.bias for lin in self.dnn.linears]
        tensors += [self.dnn_linear.weight, self.out.bias]
        logit, _, *atts = _AutoIntFn.apply(emb, dense if self.dense_dim and self.use_dnn else None, cfg, *tensors)
        for layer, att, on in zip(self.int_layers, atts, capture):
            if on:
                layer.normalized_att_scores = att
        return logit


def _esmm_fill(tgt, n_dnn, tensors):
    """Set the parameter pointers of a satrans_esmm_desc / satrans_esmm_grads from `tensors`: the layers' weights [towers, n_l,
    n_{l-1}], their biases [towers, n_l], the final weights [towers, n_last], out.bias [1]."""
    for l in range(n_dnn):
        tgt.dnn_w[l], tgt.dnn_b[l] = tensors[l].data_ptr(), tensors[n_dnn + l].data_ptr()
    tgt.final_w, tgt.out_bias = tensors[-2].data_ptr(), tensors[-1].data_ptr()
    return tgt


def _esmm_desc(x, cfg, tensors):
    """cfg = (towers, training, drop_p, seed, step, row_offset): what the backward must see as the forward saw it."""
    towers, training, drop_p, seed, step, row_offset = cfg
    n_dnn = (len(tensors) - 2) // 2
    d = _esmm_fill(N.ESMMDesc(), n_dnn, tensors)
    d.B, d.C, d.towers, d.n_dnn = x.shape[0], x.shape[1], towers, n_dnn
    for l in range(n_dnn):
        d.width[l] = tensors[n_dnn + l].shape[-1]
    d.flags, d.drop_p = (N.TRAIN if training else 0), drop_p
    d.seed, d.step, d.row_offset = seed, step, row_offset
    d.x = x.data_ptr()
    return d


class _ESMMFn(torch.autograd.Function):
    """out [B, towers] of ESMM's two towers (towers = 2: the probabilities ctr, ctcvr) or of WDL's DNN head (towers = 1: the
    logit) (csrc/esmm.hip); cfg as _esmm_desc takes it, `tensors` as _esmm_fill lists them.  `saved` = the hidden rows, then
    with two towers (p_ctr, p_cvr) [B, 2]."""

    @staticmethod
    def forward(ctx, x, cfg, *tensors):
        lib = N.lib()
        dev = x.device
        x = x.contiguous()
        tensors = tuple(t.contiguous() for t in tensors)
        d = _esmm_desc(x, cfg, tensors)
        saved = torch.empty(_native_size(lib.satrans_esmm_saved_floats, d), dtype=torch.float32, device=dev)
        out = torch.empty(x.shape[0], cfg[0], dtype=torch.float32, device=dev)
        N.check(lib.satrans_esmm_fwd(C.byref(d), out.data_ptr(), saved.data_ptr(), N.stream_handle(dev)), "satrans_esmm_fwd")
        ctx.cfg = cfg      # carries the forward's step into the backward
        ctx.save_for_backward(x, saved, *tensors)
        ctx.mark_non_differentiable(saved)
        return out, saved

    @staticmethod
    def backward(ctx, dout, _dsaved):
        lib = N.lib()
        x, saved, *tensors = ctx.saved_tensors
        d = _esmm_desc(x, ctx.cfg, tensors)
        work = torch.empty(_native_size(lib.satrans_esmm_workspace_floats, d), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(t) for t in tensors]
        g = _esmm_fill(N.ESMMGrads(), d.n_dnn, grads)
        N.check(lib.satrans_esmm_bwd(C.byref(d), dout.contiguous().data_ptr(), dx.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                     C.byref(g), N.stream_handle(x.device)), "satrans_esmm_bwd")
        return (dx, None, *grads)


class _DropoutDNNHead(nn.Module):
    """What ESMMHead and WDLHead share: the checks of the constructor and of a call, the dropout clock, the call of _ESMMFn."""

    def _init_common(self, what, inputs_dim, hidden_units, l2_reg_dnn, dnn_dropout, dnn_activation, dnn_use_bn):
        if dnn_activation != 'relu':
            raise NotImplementedError(f"{what}: activation {dnn_activation!r} is not built (relu only)")
        if dnn_use_bn:
            raise NotImplementedError(f"{what}: batch-norm inside the DNNs is not built (dnn_use_bn must be False)")
        units = [int(u) for u in hidden_units]
        if len(units) == 0:
            raise ValueError(f"{what}: the hidden units are empty (the reference has no such head)")
        if len(units) > N.MMOE_MAX_HIDDEN:
            raise NotImplementedError(f"{what}: up to MMOE_MAX_HIDDEN = {N.MMOE_MAX_HIDDEN} hidden layers, got {len(units)}")
        if inputs_dim < 1 or min(units) < 1:
            raise ValueError(f"{what}: inputs_dim and the hidden units must be positive")
        if not 0 <= dnn_dropout < 1:
            raise ValueError(f"{what}: dnn_dropout must lie in [0, 1), got {dnn_dropout}")
        self.inputs_dim, self.l2_reg_dnn, self.dnn_dropout = int(inputs_dim), float(l2_reg_dnn), float(dnn_dropout)
        self.drop_row_offset = 0
        self._clock = _DropClock()
        self._units, self.last_hidden = tuple(units), None
        return units

    def _l2(self, weights):
        total = torch.zeros((1,), device=self.out.bias.device)
        if self.l2_reg_dnn > 0:
            for p in weights:
                total = total + torch.sum(self.l2_reg_dnn * torch.square(p))
        return total

    def _run(self, what, towers, x, tensors):
        if x.dim() != 2 or x.shape[1] != self.inputs_dim:
            raise ValueError(f"{what}: expected input [B, {self.inputs_dim}], got {tuple(x.shape)}")
        N.require_gpu(x, what)
        if x.dtype != torch.float32 or self.out.bias.dtype != torch.float32:
            raise TypeError(f"{what}: rows, parameters and gradients are float32")
        if self.training:
            self._clock.step += 1
        cfg = (towers, bool(self.training), self.dnn_dropout, self._clock.seed, self._clock.step & 0xFFFFFFFF,
               int(self.drop_row_offset) & 0xFFFFFFFF)
        out, saved = _ESMMFn.apply(x, cfg, *tensors)
        B, at, self.last_hidden = x.shape[0], 0, []
        for n in self._units:      # views of the saved buffer: layer l's rows [B, towers * n_l], tower t in columns [t n_l, (t + 1) n_l)
            self.last_hidden.append(saved[at:at + B * towers * n].view(B, towers * n))
            at += B * towers * n
        return out, saved


class ESMMHead(_DropoutDNNHead):
    """The half of the reference's ESMM.forward behind the embedding lookup (models/esmm.py:84-96), sigmoids and product included:

        p_ctr = sigmoid(ctr_dnn_final_layer(ctr_dnn(x)) + out.bias),  p_cvr = sigmoid(cvr_dnn_final_layer(cvr_dnn(x)) + out.bias)
        forward(dnn_input [B, inputs_dim] fp32) -> [B, 2] = (p_ctr, p_ctr * p_cvr)                          (ctr, ctcvr)

    Probabilities, not logits: ctcvr has none.  `last_cvr` [B, 1] is the detached pCVR of the last forward, `last_hidden[l]`
    [B, 2 n_l] the hidden rows it saved (ctr_dnn's columns, then cvr_dnn's; dropped-out and scaled in training).  Two towers over all
    rows, nothing routed; the backward crosses from the product into both towers.  The whole head is ONE autograd.Function over
    satrans_esmm_fwd / satrans_esmm_bwd (csrc/esmm.hip): layer 1 of both towers one product, later layers block-diagonal, the
    final layers one product of one column per tower, then the sigmoids and the product.  Per call the two towers' parameters are stacked
    (torch.stack; autograd splits the gradients back).

    dnn_dropout: in training mode a hidden element is kept iff oracle.satrans_oracle.dropout_keep(seed, step, layer, tower, row +
    drop_row_offset, column, p) (csrc/rng.h; tower 0 = ctr_dnn, 1 = cvr_dnn) and scaled by 1 / (1 - p); the step advances with
    every training forward, and the backward sees the forward's.  Not torch's generator stream.  `drop_row_offset` (default 0)
    lets a rank or a slice keep the masks of the global batch.  eval() runs the kernels without the option.

    Parameter names, state_dict order and initialisation are the reference ESMM's: out.bias (zeros), ctr_dnn.linears.{l}.*,
    cvr_dnn.linears.{l}.* (weights N(0, init_std)), ctr_dnn_final_layer.weight, cvr_dnn_final_layer.weight - those entries of a
    reference checkpoint load with load_state_dict.  regularization_loss() -> [1] is what ESMM.__init__ registers (esmm.py:71-76).
    Not built: batch-norm and activations other than relu (NotImplementedError), more than MMOE_MAX_HIDDEN hidden layers, bf16.  Empty hidden units: ValueError (the reference indexes [-1])."""

    def __init__(self, inputs_dim, tower_dnn_hidden_units=(256, 128), l2_reg_dnn=0, init_std=0.0001, dnn_dropout=0,
                 dnn_activation='relu', dnn_use_bn=False):
        super().__init__()
        units = self._init_common("ESMMHead", inputs_dim, tower_dnn_hidden_units, l2_reg_dnn, dnn_dropout, dnn_activation, dnn_use_bn)
        self.tower_dnn_hidden_units = tuple(units)
        # (first: in the reference's state_dict `out.*` precedes ESMM's own modules, because its BaseModel registers that name)
        self.out = _OutBias()
        self.ctr_dnn = _TowerDNN(inputs_dim, units, init_std)
        self.cvr_dnn = _TowerDNN(inputs_dim, units, init_std)
        self.ctr_dnn_final_layer = nn.Linear(units[-1], 1, bias=False)
        self.cvr_dnn_final_layer = nn.Linear(units[-1], 1, bias=False)
        self.last_cvr = None

    def regularization_loss(self):
        return self._l2([lin.weight for lin in self.ctr_dnn.linears] + [lin.weight for lin in self.cvr_dnn.linears] +
                        [self.ctr_dnn_final_layer.weight, self.cvr_dnn_final_layer.weight])

    def forward(self, dnn_input):
        pairs = list(zip(self.ctr_dnn.linears, self.cvr_dnn.linears))
        tensors = ([torch.stack([a.weight, b.weight]) for a, b in pairs] + [torch.stack([a.bias, b.bias]) for a, b in pairs] +
                   [torch.cat([self.ctr_dnn_final_layer.weight, self.cvr_dnn_final_layer.weight]), self.out.bias])
        out, saved = self._run("ESMMHead", 2, dnn_input, tensors)
        B = out.shape[0]
        self.last_cvr = saved[saved.numel() - 2 * B:].view(B, 2)[:, 1:2]
        return out


class WDLHead(_DropoutDNNHead):
    """The DNN half of the reference's WDL.forward (models/wdl.py:75-77) with the bias of `self.out`:

        forward(dnn_input [B, inputs_dim] fp32) -> logit [B, 1] = dnn_linear(dnn(x)) + out.bias;  the caller keeps the sigmoid

    (wdl.py leaves linear_model out of the logit.)  ESMM's tower taken once: the same kernels at one tower (csrc/esmm.hip), ONE
    autograd.Function.  dnn_dropout, `drop_row_offset`, training / eval as in ESMMHead, with site 0 for `dnn`.  Parameter names,
    state_dict order and initialisation are the reference WDL's head entries: out.bias, dnn.linears.{l}.{weight,bias},
    dnn_linear.weight.  regularization_loss() -> [1] follows wdl.py:59-61.
    Not built: batch-norm and activations other than relu (NotImplementedError), more than MMOE_MAX_HIDDEN hidden layers, bf16, a
    WDL model class behind BaseModel.  Empty hidden units: ValueError (the reference's WDL has no DNN then)."""

    def __init__(self, inputs_dim, dnn_hidden_units=(256, 128), l2_reg_dnn=0, init_std=0.0001, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False):
        super().__init__()
        units = self._init_common("WDLHead", inputs_dim, dnn_hidden_units, l2_reg_dnn, dnn_dropout, dnn_activation, dnn_use_bn)
        self.dnn_hidden_units = tuple(units)
        self.out = _OutBias()
        self.dnn = _TowerDNN(inputs_dim, units, init_std)
        self.dnn_linear = nn.Linear(units[-1], 1, bias=False)

    def regularization_loss(self):
        return self._l2([lin.weight for lin in self.dnn.linears] + [self.dnn_linear.weight])

    def forward(self, dnn_input):
        tensors = ([lin.weight for lin in self.dnn.linears] + [lin.bias for lin in self.dnn.linears] +
                   [self.dnn_linear.weight, self.out.bias])
        logit, _ = self._run("WDLHead", 1, dnn_input, tensors)
        return logit


# ---- the front end: X -> linear_logit, emb, dense ------------------------------------------------------------------------------
_COMBINERS = {"sum": N.POOL_SUM, "mean": N.POOL_MEAN, "max": N.POOL_MAX}
EMBEDDING_DIMS = (16, 32, 64, 128)      # the widths the gather, pool and optimizer kernels are built for


class _FieldLayout:
    """The host half of a lookup over one arena: the columns split as the reference splits them, the field table of the pooled
    gather's ABI (`satrans_pool_field`: sparse fields, then varlen fields), the X columns of the dense values.  Every limit of
    the kernels is checked here, at construction, as a ValueError."""

    def __init__(self, what, feature_columns, feature_index):
        from .inputs import split_columns
        self.sparse, self.dense, self.varlen = split_columns(feature_columns)
        self.F = len(self.sparse) + len(self.varlen)
        self.Fv = len(self.varlen)
        self.R = len(self.sparse) + sum(c.maxlen for c in self.varlen)
        if self.F > N.POOL_MAX_FIELDS:
            raise ValueError(f"{what}: {self.F} sparse and varlen fields; the kernels take up to POOL_MAX_FIELDS = {N.POOL_MAX_FIELDS}")
        for c in self.varlen:
            if not 1 <= c.maxlen <= N.POOL_MAX_LEN:
                raise ValueError(f"{what}: {c.name}: maxlen {c.maxlen}; the kernels take 1..POOL_MAX_LEN = {N.POOL_MAX_LEN}")
            if c.combiner not in _COMBINERS:
                raise ValueError(f"{what}: {c.name}: combiner {c.combiner!r} is not one of {sorted(_COMBINERS)}")
        for c in self.sparse + self.varlen + self.dense:
            if c.name not in feature_index:
                raise ValueError(f"{what}: {c.name} has no columns in feature_index")
        for c in self.varlen:
            if c.length_name is not None and c.length_name not in feature_index:
                raise ValueError(f"{what}: {c.length_name} (the length of {c.name}) has no column in feature_index")
        self.names = list(dict.fromkeys(c.embedding_name for c in self.sparse + self.varlen))      # one table per embedding_name
        self.dense_cols = [j for c in self.dense for j in range(*feature_index[c.name])]
        self.n_dense = len(self.dense_cols)
        spans = [feature_index[c.name] for c in self.sparse + self.varlen + self.dense]
        spans += [feature_index[c.length_name] for c in self.varlen if c.length_name is not None]
        self.x_cols = max((hi for _, hi in spans), default=0)      # X needs this many columns
        self.feature_index = feature_index
        self.fields, self.table_rows = None, {}

    def bind(self, table_rows):
        """table_rows: embedding_name -> (first arena row, rows).  Builds the host array of satrans_pool_field."""
        fi = self.feature_index
        fields, slot = (N.PoolField * max(1, self.F))(), 0
        for f, c in enumerate(self.sparse + self.varlen):
            lo, rows = table_rows[c.embedding_name]
            fd, var = fields[f], f >= len(self.sparse)
            fd.col, fd.maxlen = fi[c.name][0], (c.maxlen if var else 1)
            fd.combiner = _COMBINERS[c.combiner] if var else N.POOL_COPY
            fd.len_col = fi[c.length_name][0] if var and c.length_name is not None else -1
            fd.slot, fd.varlen = slot, (f - len(self.sparse) if var else -1)
            fd.lo, fd.hi = lo, lo + rows
            slot += fd.maxlen
        self.fields, self.table_rows = fields, dict(table_rows)


def _input_parts(what, X, lay):
    """X: the reference's fp32 matrix, an integer id matrix (no dense columns then), or inputs.PackedInput(ids, dense).
    -> (ids [B, C] contiguous, dense matrix or None, packed: the dense values are columns 0..n_dense-1 of `dense`)."""
    from .inputs import PackedInput
    packed = isinstance(X, PackedInput)
    ids, dense = (X.ids, X.dense) if packed else (X, X)
    if not torch.is_tensor(ids) or ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < lay.x_cols:
        raise ValueError(f"{what}: expected X [B, >= {lay.x_cols}], got {tuple(ids.shape) if torch.is_tensor(ids) else type(ids)}")
    N.require_gpu(ids, what)
    N.id_dtype_of(ids)
    if not packed and ids.dtype != torch.float32:
        dense = None
    if lay.n_dense:
        if dense is None or dense.dtype != torch.float32:
            raise TypeError(f"{what}: the dense columns need a float32 X or a PackedInput with a float32 dense block")
        if packed and (dense.dim() != 2 or tuple(dense.shape) != (ids.shape[0], lay.n_dense) or dense.device != ids.device):
            raise ValueError(f"{what}: PackedInput.dense must be [{ids.shape[0]}, {lay.n_dense}] beside the ids, got {tuple(dense.shape)}")
        dense = dense.contiguous()
    else:
        dense = None
    return ids.contiguous(), dense, packed


class _TableArena:
    """What LinearModel and FeatureEmbedding share: the tables of `embedding_dict` as views of ONE arena (rebuilt after every
    `.to()`, as BaseModel._rebind_storage), the field table over it, the device-side column lists and the status word."""

    def _rebind_storage(self):
        lay = self._layout
        tables = [self.embedding_dict[n].weight for n in lay.names]
        rows, off = OrderedDict(), 0
        for n, t in zip(lay.names, tables):
            rows[n] = (off, t.shape[0])
            off += t.shape[0]
        self.arena = None
        dev = tables[0].device if tables else (self.weight.device if getattr(self, "weight", None) is not None else torch.device("cpu"))
        if tables:
            self.arena = torch.cat([t.data.reshape(t.shape[0], -1) for t in tables], dim=0).contiguous()
            for n, t in zip(lay.names, tables):
                lo, cnt = rows[n]
                t.data = self.arena[lo:lo + cnt]
        lay.bind(rows)
        i32 = dict(dtype=torch.int32, device=dev)
        self._dense_cols_x = torch.tensor(lay.dense_cols, **i32)
        self._dense_cols_packed = torch.arange(lay.n_dense, **i32)
        self._status = torch.zeros(1, **i32)
        sp = [f for f in lay.fields[:lay.F]]
        self._gather_cols = torch.tensor([f.col for f in sp], **i32)
        self._row_span = torch.tensor([[f.lo, f.hi] for f in sp], dtype=torch.int64, device=dev).reshape(-1, 2)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if getattr(self, "_layout", None) is not None:
            self._rebind_storage()
        return out

    def _tables(self):
        """The tables in arena order, still views of the arena (a `.data` assignment from outside is folded back in)."""
        lay = self._layout
        tables = [self.embedding_dict[n].weight for n in lay.names]
        width = self.arena.shape[1] * 4
        if any(t.data_ptr() != self.arena.data_ptr() + lay.table_rows[n][0] * width for n, t in zip(lay.names, tables)):
            self._rebind_storage()
        return tables

    def _raise_on_status(self, what):
        """One device-to-host read per forward; the word is cleared before raising, so the next call starts clean."""
        flags = int(self._status.item())
        if flags:
            self._status.zero_()
            if flags & 1:
                raise IndexError(f"index out of range in self: {what}: an id lies outside its table")
            raise N.NativeError(f"{what}: a dense column lies outside the dense matrix")

    def _table_grads(self, g_arena):
        return [g_arena[lo:lo + cnt] for lo, cnt in (self._layout.table_rows[n] for n in self._layout.names)]


def _sorted_positions(lib, rows, n, arena_rows, dev):
    """satrans_embed_sort over the n slot rows of a batch -> (sorted_rows, src), equal rows in position order."""
    i32 = dict(dtype=torch.int32, device=dev)
    sorted_rows, src = torch.empty(n, **i32), torch.empty(n, **i32)
    nbytes = int(lib.satrans_embed_sort_workspace_bytes(n, arena_rows))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    N.check(lib.satrans_embed_sort(rows.data_ptr(), n, arena_rows, sorted_rows.data_ptr(), src.data_ptr(), None, ws.data_ptr(),
                                   ws.numel(), None, N.stream_handle(dev)), "satrans_embed_sort")
    return sorted_rows, src


def _linear_desc(mod, ids, dense, packed, weight):
    lay = mod._layout
    d = N.LinearDesc()
    d.B, d.F, d.R, d.Fv = ids.shape[0], lay.F, lay.R, lay.Fv
    d.id_dtype, d.n_dense = N.id_dtype_of(ids), lay.n_dense
    d.x_stride, d.arena_rows = ids.shape[1], (mod.arena.shape[0] if mod.arena is not None else 0)
    d.arena = mod.arena.data_ptr() if mod.arena is not None else None
    d.fields = C.cast(lay.fields, C.POINTER(N.PoolField)) if lay.F else None
    d.X = ids.data_ptr()
    if lay.n_dense:
        d.dense, d.dense_stride = dense.data_ptr(), dense.shape[1]
        d.dense_cols = (mod._dense_cols_packed if packed else mod._dense_cols_x).data_ptr()
        d.weight = weight.data_ptr()
    return d


class _LinearFn(torch.autograd.Function):
    """linear_logit [B, 1] of LinearModel (csrc/linear.hip).  `params`: the tables in arena order (views of mod.arena, which the
    kernels read), then `weight` when there are dense columns; their gradients: slices of one zero-filled [arena_rows, 1] buffer,
    and dweight.  Adopted by an optim.TableAdam: the lazy 1-wide form first replays the batch's slot rows; the backward stores the
    row sums into the optimizer's buffer, hands it (sorted_rows, dweight) and returns no gradient."""

    @staticmethod
    def forward(ctx, mod, ids, dense, packed, *params):
        lib = N.lib()
        dev, lay = ids.device, mod._layout
        B = ids.shape[0]
        weight = params[-1].contiguous() if lay.n_dense else None
        d = _linear_desc(mod, ids, dense, packed, weight)
        rec = getattr(mod, "_table_opt", None)
        if rec is not None:
            rec.check_device()
            if rec.lazy:
                rec.replay_linear(d)
        logit = torch.empty(B, 1, dtype=torch.float32, device=dev)
        rows = torch.empty(B, lay.R, dtype=torch.int32, device=dev)
        mask = torch.empty(B, lay.Fv, dtype=torch.int32, device=dev)
        argmax = torch.empty(B, lay.Fv, dtype=torch.uint8, device=dev)
        N.check(lib.satrans_linear_fwd(C.byref(d), logit.data_ptr(), rows.data_ptr(), mask.data_ptr(), argmax.data_ptr(),
                                       mod._status.data_ptr(), N.stream_handle(dev)), "satrans_linear_fwd")
        mod._raise_on_status("LinearModel")
        ctx.mod, ctx.packed, ctx.ids, ctx.dense = mod, packed, ids, dense
        ctx.rec, ctx.fwd_t = rec, (rec.opt.t if rec is not None else 0)
        ctx.save_for_backward(rows, mask, argmax, *([weight] if lay.n_dense else []))
        return logit

    @staticmethod
    def backward(ctx, dlogit):
        lib = N.lib()
        mod, lay, ids = ctx.mod, ctx.mod._layout, ctx.ids
        rows, mask, argmax, *w = ctx.saved_tensors
        dev = ids.device
        d = _linear_desc(mod, ids, ctx.dense, ctx.packed, w[0] if w else None)
        dlogit = dlogit.contiguous().float()
        f32 = dict(dtype=torch.float32, device=dev)
        g_arena = sorted_rows = src = dweight = None
        rec = ctx.rec
        if rec is not None:
            rec.refuse_second()
        if lay.F:
            sorted_rows, src = _sorted_positions(lib, rows, rows.numel(), d.arena_rows, dev)
            if rec is None:
                g_arena = torch.zeros(d.arena_rows, 1, **f32)
            else:                                     # the optimizer's buffer: all-zero already in the lazy form (its step clears
                g_arena = rec.g                       # the rows written here), cleared here for the dense sweep
                if not rec.lazy:
                    g_arena.zero_()
        if lay.n_dense:
            dweight = torch.empty(lay.n_dense, 1, **f32)
        work = torch.empty(max(256, _native_size(lib.satrans_linear_workspace_bytes, d)), dtype=torch.uint8, device=dev)
        N.check(lib.satrans_linear_bwd(C.byref(d), dlogit.data_ptr(), rows.data_ptr(), mask.data_ptr(), argmax.data_ptr(),
                                       N.ptr(sorted_rows), N.ptr(src), N.ptr(g_arena), N.ptr(dweight), work.data_ptr(),
                                       N.stream_handle(dev)), "satrans_linear_bwd")
        if rec is not None:
            rec.take(sorted_rows, src, dweight, rows.numel(), ctx.fwd_t)
            return (None,) * (4 + len(mod._layout.names) * bool(lay.F) + bool(lay.n_dense))
        grads = (mod._table_grads(g_arena) if lay.F else []) + ([dweight] if lay.n_dense else [])
        return (None, None, None, None, *grads)


class LinearModel(_TableArena, _LinearTables):
    """deepctr's `Linear`, the order-1 term `linear_model(X)` of the reference's WDL, DCN, DeepFM, xDeepFM, NFM, AFM and FiBiNET
    (models/meta_basemodel.py:34-92):

        forward(X) -> linear_logit [B, 1] = sum over the sparse fields, then the pooled varlen fields, of their 1-wide
                      embeddings + cat(dense values) @ weight

    X is the reference's fp32 matrix in `feature_index` column order, or inputs.PackedInput(ids, dense) (integer ids; `dense`
    holds this module's dense values in concatenation order), or a bare integer matrix when there is no DenseFeat.  ONE
    autograd.Function over satrans_linear_fwd / satrans_linear_bwd (csrc/linear.hip): one launch forward - the summation order is
    fixed (fields in the reference's list order, then the dense products ascending, fp32; satrans_hip.h) and a sample's logit
    does not depend on its batch - and, backward, satrans_embed_sort plus an ordered segment sum without float atomics: the same
    call twice gives the same bits.  The pooling rules are the pooled gather's (sum / mean / max, mask by the length column or
    by id != 0).  An id outside its table raises IndexError from the forward (one status read per call).

    Parameters, their creation order and the generator draws are the reference's (`_LinearTables`: the tables drawn twice,
    then `weight`): state_dict keys `embedding_dict.<embedding_name>.weight` [V, 1] and `weight` [n_dense, 1] (absent without a
    DenseFeat); fields sharing an embedding_name share one parameter.  The tables are views of one 1-wide arena (`self.arena`),
    rebound after `.to()`.  This is the reference's sparse=False semantics: every table receives a DENSE gradient, a slice of one
    zero-filled [rows, 1] buffer, so any torch optimizer trains it.  Adopted by an optim.TableAdam, the backward stores the row
    sums into a buffer the optimizer owns, every `.grad` stays None, and the optimizer steps the tables (one satrans_adam_flat
    sweep, or the lazy 1-wide kernels with `linear_lazy=True`) and `weight`.  Without sparse and varlen columns the result is the
    dense term alone; without dense columns there is no `weight`; with neither, zeros [B, 1] (the reference's).
    Not built: `sparse_feat_refine_weight` (IFM / DIFM; NotImplementedError - the reference never passes it), sparse-COO
    gradients, bf16, one sort shared with FeatureEmbedding."""

    def __init__(self, feature_columns, feature_index, init_std=0.0001, device='cpu'):
        lay = _FieldLayout("LinearModel", feature_columns, feature_index)      # (refuses before a generator draw is made)
        super().__init__(feature_columns, init_std)
        self.feature_index, self.device = feature_index, device
        self.sparse_feature_columns, self.dense_feature_columns = lay.sparse, lay.dense
        self.varlen_sparse_feature_columns = lay.varlen
        self._layout = lay
        self._rebind_storage()
        self.to(device)

    def forward(self, X, sparse_feat_refine_weight=None):
        if sparse_feat_refine_weight is not None:
            raise NotImplementedError("LinearModel: sparse_feat_refine_weight (IFM / DIFM) is not built")
        lay = self._layout
        if lay.F == 0 and lay.n_dense == 0:
            ids = X.ids if not torch.is_tensor(X) else X
            return torch.zeros(ids.shape[0], 1, dtype=torch.float32, device=ids.device)
        ids, dense, packed = _input_parts("LinearModel", X, lay)
        params = (self._tables() if lay.F else []) + ([self.weight] if lay.n_dense else [])
        if any(p.dtype != torch.float32 for p in params):
            raise TypeError("LinearModel: tables, weight and gradients are float32")
        if any(p.device != ids.device for p in params):
            raise N.NativeError(f"LinearModel: X is on {ids.device}, the parameters on {params[0].device}")
        return _LinearFn.apply(self, ids, dense, packed, *params)


class _FeatureEmbeddingFn(torch.autograd.Function):
    """emb [B, F, D] of FeatureEmbedding over the existing ABI: satrans_gather_fwd (no varlen column) or satrans_pool_gather_fwd;
    backward satrans_pool_bwd (varlen only), satrans_embed_sort, then the dense gradient into a zero-filled [rows, D] by
    satrans_embed_segment_sums or satrans_embed_grad_dense(l2 = 0) (FeatureEmbedding.dense_gradient).
    Adopted by an optim.TableAdam: the lazy form runs a rows-only pass, the sort and satrans_embed_lazy_replay of exactly these
    rows in front of the gather (the sort is kept for the backward); the backward stops after the sort, hands (sorted_rows, src,
    gemb) to the optimizer and returns no gradient - the [rows, D] buffer is never built."""

    @staticmethod
    def forward(ctx, mod, ids, *tables):
        lib = N.lib()
        dev, lay, arena = ids.device, mod._layout, mod.arena
        B, D = ids.shape[0], arena.shape[1]
        emb = torch.empty(B, lay.F, D, dtype=torch.float32, device=dev)
        rows = torch.empty(B, lay.R, dtype=torch.int32, device=dev)
        mask = argmax = None
        st = N.stream_handle(dev)
        rec, presorted = getattr(mod, "_table_opt", None), None
        if rec is not None:
            rec.check_device()
        if rec is not None and rec.lazy:      # rows only (an id outside its table counts as its first row: the replay is neutral)
            if lay.Fv == 0:
                N.check(lib.satrans_gather_fwd(arena.data_ptr(), mod._row_span.data_ptr(), mod._gather_cols.data_ptr(),
                                               ids.data_ptr(), N.id_dtype_of(ids), ids.shape[1], B, lay.F, D, None, rows.data_ptr(),
                                               mod._status.data_ptr(), st), "satrans_gather_fwd(rows)")
            else:
                N.check(lib.satrans_pool_gather_fwd(arena.data_ptr(), arena.shape[0], None, None, lay.fields, lay.F, lay.R, lay.Fv,
                                                    ids.data_ptr(), N.id_dtype_of(ids), ids.shape[1], B, D, None, rows.data_ptr(),
                                                    None, None, mod._status.data_ptr(), st), "satrans_pool_gather_fwd(rows)")
            presorted = _sorted_positions(lib, rows, B * lay.R, arena.shape[0], dev)
            rec.replay(presorted[0], B * lay.R)
        if lay.Fv == 0:
            N.check(lib.satrans_gather_fwd(arena.data_ptr(), mod._row_span.data_ptr(), mod._gather_cols.data_ptr(), ids.data_ptr(),
                                           N.id_dtype_of(ids), ids.shape[1], B, lay.F, D, emb.data_ptr(), rows.data_ptr(),
                                           mod._status.data_ptr(), st), "satrans_gather_fwd")
        else:
            mask = torch.empty(B, lay.Fv, dtype=torch.int32, device=dev)
            argmax = torch.empty(int(lib.satrans_pool_argmax_bytes(B, lay.Fv, D)), dtype=torch.uint8, device=dev)
            N.check(lib.satrans_pool_gather_fwd(arena.data_ptr(), arena.shape[0], None, None, lay.fields, lay.F, lay.R, lay.Fv,
                                                ids.data_ptr(), N.id_dtype_of(ids), ids.shape[1], B, D, emb.data_ptr(),
                                                rows.data_ptr(), mask.data_ptr(), argmax.data_ptr(), mod._status.data_ptr(), st),
                    "satrans_pool_gather_fwd")
        mod._raise_on_status("FeatureEmbedding")
        ctx.mod = mod
        ctx.rec, ctx.presorted, ctx.fwd_t = rec, presorted, (rec.opt.t if rec is not None else 0)
        ctx.save_for_backward(rows, *([mask, argmax] if lay.Fv else []))
        return emb

    @staticmethod
    def backward(ctx, demb):
        lib = N.lib()
        mod, lay, arena = ctx.mod, ctx.mod._layout, ctx.mod.arena
        rows, *pooled = ctx.saved_tensors
        dev, st = rows.device, N.stream_handle(rows.device)
        B, D, total = rows.shape[0], arena.shape[1], arena.shape[0]
        rec = ctx.rec
        if rec is not None:
            rec.refuse_second()
        gemb = demb.contiguous().float()
        if lay.Fv:
            dx, gemb = gemb, torch.empty(B * lay.R, D, dtype=torch.float32, device=dev)
            N.check(lib.satrans_pool_bwd(dx.data_ptr(), lay.fields, lay.F, lay.R, lay.Fv, B, D, pooled[0].data_ptr(),
                                         pooled[1].data_ptr(), gemb.data_ptr(), st), "satrans_pool_bwd")
        n = B * lay.R
        sorted_rows, src = ctx.presorted if ctx.presorted is not None else _sorted_positions(lib, rows, n, total, dev)
        if rec is not None:
            rec.take(sorted_rows, src, gemb, n, ctx.fwd_t)
            return (None,) * (2 + len(lay.names))
        g_arena = torch.zeros(total, D, dtype=torch.float32, device=dev)
        if mod.dense_gradient == "segment_sums":      # the engine's chunked ordered sums, stored instead of applied
            part = torch.empty(int(lib.satrans_embed_partial_ws_floats(n, D)), dtype=torch.float32, device=dev)
            unused = torch.empty(int(lib.satrans_embed_reg_partials(total, n, D)), dtype=torch.float64, device=dev)
            N.check(lib.satrans_embed_segment_sums(sorted_rows.data_ptr(), src.data_ptr(), n, gemb.data_ptr(), D, part.data_ptr(),
                                                   unused.data_ptr(), g_arena.data_ptr(), st), "satrans_embed_segment_sums")
        else:                                         # one lane group per run, walked in position order
            N.check(lib.satrans_embed_grad_dense(arena.data_ptr(), sorted_rows.data_ptr(), src.data_ptr(), n, gemb.data_ptr(), total,
                                                 D, 0.0, g_arena.data_ptr(), st), "satrans_embed_grad_dense")
        return (None, None, *mod._table_grads(g_arena))


class FeatureEmbedding(_TableArena, nn.Module):
    """The reference's `input_from_feature_columns` (models/meta_basemodel.py:519-545) as one module - what every sibling head
    starts from:

        forward(X) -> (emb [B, F, D] fp32, dense [B, n_dense] fp32 or None)      F = the sparse fields, then the varlen fields

    `embedding_dict` is `make_embedding_tables`' (the reference's keys, generator draws and sharing by embedding_name; state_dict
    keys `embedding_dict.<embedding_name>.weight`); the tables are views of one arena [rows, D] (`self.arena`), rebound after
    `.to()`.  No kernel of its own: ONE autograd.Function over the existing ABI - satrans_gather_fwd without varlen columns (every
    element a copy: bit-exact), else satrans_pool_gather_fwd; backward satrans_pool_bwd (varlen only), satrans_embed_sort, and
    the per-row sums of the sorted gradient rows stored into the dense buffer - no float atomics, the same bits every run.
    `dense_gradient` picks the kernel of that last step: "segment_sums" (default; satrans_embed_segment_sums, the engine's
    chunked ordered sums, which split a row that thousands of samples gather) or "grad_dense" (satrans_embed_grad_dense, one
    lane group walking each row's run in position order: 2.6 ms against 0.41 ms, and the torch form's 2.1 ms, at AliCCP shape, where four
    fields have 4 to 15 ids for 8192 samples; profiles/input_time.txt).  `dense` is the X columns of the DenseFeats
    (PackedInput.dense as it is) and carries no gradient; X as in LinearModel.  An id outside its table raises IndexError.

    This is the reference's sparse=False semantics: every table's gradient is DENSE, a slice of one zero-filled [rows, D] buffer
    in which every row exists.  At AliCCP size (about 6.6 M rows) that buffer is 0.84 GB at D = 32: it is zero-filled and
    written every backward and read again, with two moment buffers of the same size, by a dense optimizer step - against a few
    MB of gathered rows.  optim.TableAdam removes both: an adopted module's forward first replays the postponed steps of the
    batch's rows (also under no_grad and in eval()), its backward hands (sorted_rows, src, gemb) to the optimizer instead of
    building the buffer - every `.grad` stays None - and the step touches gathered rows only (profiles/table_adam_time.txt).
    Between steps `embedding_dict[...].weight` then shows postponed rows as they were left; `state_dict()` flushes first.
    embedding_dim must be one of {16, 32, 64, 128} and the same for every field, at most POOL_MAX_FIELDS fields and
    POOL_MAX_LEN slots per list: ValueError at construction.
    Not built: sparse-COO gradients, bf16, one sort shared with LinearModel, baseline model classes behind BaseModel."""

    def __init__(self, feature_columns, feature_index, init_std=0.0001, device='cpu'):
        lay = _FieldLayout("FeatureEmbedding", feature_columns, feature_index)
        if lay.F == 0:
            raise ValueError("FeatureEmbedding: no SparseFeat or VarLenSparseFeat column (there is no emb to return)")
        dims = sorted({c.embedding_dim for c in lay.sparse + lay.varlen})
        if len(dims) != 1 or dims[0] not in EMBEDDING_DIMS:
            raise ValueError(f"FeatureEmbedding: embedding_dim {dims} must be one value of {{16, 32, 64, 128}} for every field")
        super().__init__()
        self.feature_index, self.device = feature_index, device
        self.embedding_size = dims[0]
        self.dense_gradient = "segment_sums"
        self.embedding_dict = make_embedding_tables(feature_columns, init_std)
        self._layout = lay
        self._rebind_storage()
        self.to(device)

    def forward(self, X):
        from .inputs import PackedInput
        lay = self._layout
        ids, dense, packed = _input_parts("FeatureEmbedding", X, lay)
        tables = self._tables()
        if any(t.dtype != torch.float32 for t in tables):
            raise TypeError("FeatureEmbedding: tables and gradients are float32")
        if tables[0].device != ids.device:
            raise N.NativeError(f"FeatureEmbedding: X is on {ids.device}, the tables on {tables[0].device}")
        emb = _FeatureEmbeddingFn.apply(self, ids, *tables)
        if dense is not None and not packed:
            lo = lay.dense_cols[0]
            contiguous = lay.dense_cols == list(range(lo, lo + lay.n_dense))
            dense = dense[:, lo:lo + lay.n_dense] if contiguous else dense.index_select(1, self._dense_cols_x.long())
        return emb, (dense.detach() if dense is not None else None)


# ---- the tail of a step: prediction, loss, the loss's gradient -------------------------------------------------------------------
PRED_KINDS = {"binary": 0, "regression": 1}                              # SATRANS_PRED_SIGMOID / SATRANS_PRED_LINEAR
LOSS_KINDS = {"binary_crossentropy": 0, "mse": 1, "mae": 2}              # SATRANS_LOSS_*


def _point_loss_launch(logit, y, pred_kind, loss_kind, want_dz):
    """One satrans_point_loss call over the first column of `logit` [B] / [B, T] -> (loss_sum [] fp64 or None, pred [B, 1], dz)."""
    lib, dev, B = N.lib(), logit.device, logit.shape[0]
    pred = torch.empty(B, 1, dtype=torch.float32, device=dev)
    loss = dz = part = None
    if y is not None:
        loss = torch.zeros((), dtype=torch.float64, device=dev)
        part = torch.empty(max(int(lib.satrans_point_loss_partials(B)), 1), dtype=torch.float64, device=dev)
        if want_dz:
            dz = torch.empty(B, dtype=torch.float32, device=dev)
    N.check(lib.satrans_point_loss(logit.data_ptr(), logit.stride(0), N.ptr(y), B, pred_kind, loss_kind, pred.data_ptr(), N.ptr(dz),
                                   N.ptr(loss), N.ptr(part), N.stream_handle(dev)), "satrans_point_loss")
    return loss, pred, dz


class _PointLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, y, pred_kind, loss_kind):
        want = ctx.needs_input_grad[0]
        loss, pred, dz = _point_loss_launch(logit, y, pred_kind, loss_kind, want)
        ctx.shape = logit.shape
        if want:
            ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, grad_loss, _grad_pred):
        dz, = ctx.saved_tensors
        return (grad_loss.to(torch.float32) * dz).view(ctx.shape), None, None, None


class PointLoss(nn.Module):
    """The tail of the sibling models' training step in one call (csrc/point_loss.hip): PredictionLayer's sigmoid (task='binary')
    or identity ('regression'), the loss of compile() with reduction='sum' (reference models/basemodel.py:299-315), and the
    gradient of that sum at the logit.

        forward(logit [B, 1] or [B] fp32, y [B] / [B, 1] fp32) -> (loss_sum: 0-dim float64 on the device, pred [B, 1] fp32)
        forward(logit)                                          -> (None, pred [B, 1])

    The arithmetic per sample is head.hip's (`pred` and the gradient equal satrans_head_loss's prob and dlogit bit for bit); the
    sum widens every fp32 loss to double and adds them in a fixed order: the same bits every run.  ONE autograd.Function: the
    backward is `grad_loss * dz` with the dz the forward launch wrote (not written when the logit needs no gradient); `pred`
    carries no gradient.  'regression' with binary_crossentropy takes the logit itself as the probability, as the reference would."""

    def __init__(self, loss="binary_crossentropy", task="binary"):
        super().__init__()
        if task not in PRED_KINDS:
            raise ValueError("task must be binary or regression")
        if loss not in LOSS_KINDS:
            raise NotImplementedError(str(loss))
        self.loss, self.task = loss, task

    def forward(self, logit, y=None):
        N.require_gpu(logit, "PointLoss")
        if logit.dtype != torch.float32 or logit.dim() not in (1, 2) or (logit.dim() == 2 and logit.shape[1] != 1) or logit.shape[0] < 1:
            raise ValueError(f"PointLoss: expected a float32 logit [B, 1] or [B], got {logit.dtype} {tuple(logit.shape)}")
        logit = logit.contiguous()
        if y is not None:
            if y.numel() != logit.shape[0] or y.device != logit.device:
                raise ValueError(f"PointLoss: {logit.shape[0]} logits on {logit.device}, labels {tuple(y.shape)} on {y.device}")
            y = y.reshape(-1).to(torch.float32).contiguous()
        pk, lk = PRED_KINDS[self.task], LOSS_KINDS[self.loss]
        if y is None or not torch.is_grad_enabled():
            loss, pred, _ = _point_loss_launch(logit.detach(), y, pk, lk, False)
            return loss, pred
        return _PointLossFn.apply(logit, y, pk, lk)


def _routed_loss_launch(z, task, y, pred_kind, loss_kind, want_dz):
    """One satrans_point_loss_routed call over z [B, T] -> (loss_sum [] fp64 or None, pred [B, 1], dz [B, T] or None)."""
    lib, dev, (B, T) = N.lib(), z.device, z.shape
    pred = torch.empty(B, 1, dtype=torch.float32, device=dev)
    loss = dz = part = None
    if y is not None:
        loss = torch.zeros((), dtype=torch.float64, device=dev)
        part = torch.empty(max(int(lib.satrans_point_loss_partials(B)), 1), dtype=torch.float64, device=dev)
        if want_dz:
            dz = torch.empty(B, T, dtype=torch.float32, device=dev)      # (the kernel writes every entry)
    N.check(lib.satrans_point_loss_routed(z.data_ptr(), z.stride(0), task.data_ptr(), N.ptr(y), B, T, pred_kind, loss_kind,
                                          pred.data_ptr(), N.ptr(dz), N.ptr(loss), N.ptr(part), N.stream_handle(dev)),
            "satrans_point_loss_routed")
    return loss, pred, dz


class _RoutedPointLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, task, y, pred_kind, loss_kind):
        want = ctx.needs_input_grad[0]
        loss, pred, dz = _routed_loss_launch(z, task, y, pred_kind, loss_kind, want)
        if want:
            ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, grad_loss, _grad_pred):
        dz, = ctx.saved_tensors
        return grad_loss.to(torch.float32) * dz, None, None, None, None


class RoutedPointLoss(nn.Module):
    """PointLoss over a [B, T] block of per-task outputs, each row on the column of its own task (csrc/point_loss.hip,
    satrans_point_loss_routed): the multi-task models' masked per-task loss sum (reference models/mtl_basemodel.py:268-269) and
    their predict assembly (:376-378) in one launch plus the fixed-order reduction.

        forward(z [B, T] fp32, task_ids [B] integer, y [B] / [B, 1] fp32) -> (loss_sum: 0-dim float64 on the device, pred [B, 1])
        forward(z, task_ids)                                              -> (None, pred [B, 1])

    `task_ids` are columns (scenario id minus domain_id_offset).  A row whose task lies in [0, T) carries PointLoss's bits for
    z[b, task]: pred, the gradient at dz[b, task], its term of the sum.  Any other row belongs to no task, as in the reference:
    pred 0, no loss, no gradient.  ONE autograd.Function: the backward is `grad_loss * dz` with the [B, T] dz the forward launch
    wrote in full.  z may have any row stride (unit column stride); `pred` carries no gradient.  For a head that returns
    probabilities (ESMMHead) take task='regression'."""

    def __init__(self, loss="binary_crossentropy", task="binary"):
        super().__init__()
        if task not in PRED_KINDS:
            raise ValueError("task must be binary or regression")
        if loss not in LOSS_KINDS:
            raise NotImplementedError(str(loss))
        self.loss, self.task = loss, task

    def forward(self, z, task_ids, y=None):
        N.require_gpu(z, "RoutedPointLoss")
        if z.dtype != torch.float32 or z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1:
            raise ValueError(f"RoutedPointLoss: expected float32 z [B, T], got {z.dtype} {tuple(z.shape)}")
        B = z.shape[0]
        if z.stride(1) != 1 or z.stride(0) < z.shape[1]:
            z = z.contiguous()
        if task_ids.numel() != B or task_ids.device != z.device or task_ids.is_floating_point():
            raise ValueError(f"RoutedPointLoss: {B} rows on {z.device}, task ids {task_ids.dtype} {tuple(task_ids.shape)} on "
                             f"{task_ids.device}")
        task_ids = task_ids.reshape(-1).to(torch.int32).contiguous()
        if y is not None:
            if y.numel() != B or y.device != z.device:
                raise ValueError(f"RoutedPointLoss: {B} rows on {z.device}, labels {tuple(y.shape)} on {y.device}")
            y = y.reshape(-1).to(torch.float32).contiguous()
        pk, lk = PRED_KINDS[self.task], LOSS_KINDS[self.loss]
        if y is None or not torch.is_grad_enabled():
            loss, pred, _ = _routed_loss_launch(z.detach(), task_ids, y, pk, lk, False)
            return loss, pred
        return _RoutedPointLossFn.apply(z, task_ids, y, pk, lk)
