/*
 * satrans_hip.h  --  C ABI of libsatrans_hip.so, the MI355X (gfx950) implementation of the
 * SATrans scenario-adaptive attention path.
 *
 * The reference (qwerfdsaplking/SATrans) is pure Python on PyTorch: it has no FFI of its own, so
 * the boundary a maintainer binds is the set of tensor-level operations its `SATrans.forward`,
 * `BaseModel.fit` and `torch.optim.Adam` perform for this path.  Each entry point below names the
 * reference lines it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions (all entry points):
 *   - plain C types only; every pointer is a DEVICE pointer unless its name starts with `h_`;
 *   - the caller owns all memory, passes workspaces in, and keeps buffers alive until the stream
 *     has executed the call; nothing here allocates, frees or synchronises;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); every kernel is enqueued on
 *     it, so calls are re-entrant per stream and capturable into a hipGraph;
 *   - return value: 0 on success, a negative SATRANS_E_* code otherwise; nothing throws across
 *     the ABI.  `satrans_last_error()` returns a static description of the last failure of the
 *     calling thread.
 *   - tensors are dense row-major fp32 unless stated; sizes are in elements.
 */
#ifndef SATRANS_HIP_H
#define SATRANS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: satrans_layer_desc gained the trailing `attn_save` field and satrans_set_layer_bwd8 left the library (round 3; the number
 *    was bumped one round late); round 4 added satrans_layer_bwd_head (a new entry point, no struct changed).  A caller built against an
 *    older header passes a shorter struct: satrans_abi_version() must be compared with this constant before any other call. */
/* 6: satrans_adam_hparams gained the trailing `arith` field (round 6). */
/* 7: the scenario attention statistics (satrans_attn_stats_workspace_bytes, satrans_attn_stats_accumulate); no struct changed. */
/*    Also in 7, added later: the pooled gather of VarLenSparseFeat fields and its backward (satrans_pool_field,
 *    satrans_pool_gather_fwd, satrans_pool_bwd, satrans_pool_argmax_bytes).  Purely additive - no existing struct or entry point
 *    changed - so a caller built against the earlier version-7 header runs unchanged; the binding checks the new symbols at load.
 *    Likewise the instance-level attention search (satrans_attn_rule, satrans_attn_match, satrans_attn_inst_*) and the
 *    partitioned normalisation (satrans_pnorm_desc, satrans_pnorm_*), and after it STAR's star-topology towers
 *    (satrans_star_desc, satrans_star_*), the scenario-routed MMoE head (satrans_mmoe_desc, satrans_mmoe_*) and the
 *    scenario-routed PLE head (satrans_ple_desc, satrans_ple_grads, satrans_ple_*), and AdaSparse's scenario-pruned DNN
 *    (satrans_adasparse_desc, satrans_adasparse_grads, satrans_adasparse_*), and the scenario-routed SharedBottom head
 *    (satrans_sharedbottom_desc, satrans_sharedbottom_grads, satrans_sharedbottom_*), and xDeepFM's compressed interaction
 *    network (satrans_cin_desc, satrans_cin_grads, satrans_cin_*), and DCN's cross network (satrans_cross_desc,
 *    satrans_cross_grads, satrans_cross_*), and FiBiNET's SENet, bilinear interaction and head (satrans_senet_*,
 *    satrans_bilinear_*, satrans_fibinet_*), and PNN's inner and outer product layers and head (satrans_inner_product_*,
 *    satrans_outer_product_*, satrans_pnn_*), and FM, BiInteractionPooling, AFM and the DeepFM / NFM heads (satrans_fm_*,
 *    satrans_bipool_*, satrans_afm_*, satrans_fmhead_*), and AutoInt's interacting layer and head (satrans_interacting_*,
 *    satrans_autoint_*), and ESMM's two towers and WDL's DNN head with dropout (satrans_esmm_desc, satrans_esmm_grads,
 *    satrans_esmm_*), and the prediction + loss + gradient of a logit column (satrans_point_loss,
 *    satrans_point_loss_partials) and its routed form over a [B, T] block (satrans_point_loss_routed), and the lazy replay and flush with the regulariser's sums in the step kernels'
 *    arithmetic (satrans_embed_lazy_replay_reg64, satrans_embed_lazy_flush_reg64). */
#define SATRANS_ABI_VERSION 7

/* error codes */
#define SATRANS_OK 0
#define SATRANS_E_BADARG (-1)      /* null pointer, negative size, unsupported dtype code          */
#define SATRANS_E_UNSUPPORTED (-2) /* shape outside what the kernels are built for (see below)     */
#define SATRANS_E_LAUNCH (-3)      /* hipLaunch / runtime error                                    */
#define SATRANS_E_WORKSPACE (-4)   /* workspace too small                                          */

/* id dtypes accepted wherever ids are read out of the input matrix X */
#define SATRANS_ID_F32 0 /* ids carried as floats and truncated, reference meta_basemodel.py:311,533-535 */
#define SATRANS_ID_I32 1
#define SATRANS_ID_I64 2

/* layer flags (bit mask) */
#define SATRANS_META_Q 1    /* 'Q' in meta_mode: MetaNet on the query projection, satrans.py:60-66     */
#define SATRANS_META_K 2    /* 'K' in meta_mode: MetaNet on the key projection,   satrans.py:67-73     */
#define SATRANS_RELU_OUT 4  /* flag 'relu': ReLU after Out_linear,                 satrans.py:91-92     */
#define SATRANS_NO_RES 8    /* att_res=False                                                           */
#define SATRANS_TRAIN 16    /* apply the four dropouts (p = drop_p)                                    */
#define SATRANS_GATE 32     /* flag 'gate': q,k *= 2*vec instead of the MetaNet,   satrans.py:61-62,68-69 */
#define SATRANS_BILINEAR 64 /* flag 'bilinear': per-head q_h @ M[s,h],             satrans.py:79-81     */
/* General path only (satrans_layer_fwd_generic / satrans_layer_bwd_generic; every other entry point refuses them): a stack of
 * layers (satrans.py:236-239: `for layer in self.domain_int_layers`) keeps its activations in the scenario-sorted order of
 * d->order between its layers instead of changing the order at both ends of every layer.
 *   X_SORTED  x (and, in the backward, dx) are rows [position in d->order][F][D]; x is not copied: the backward reads d->x again
 *   Y_SORTED  y (and, in the backward, dy) likewise */
#define SATRANS_X_SORTED 128
#define SATRANS_Y_SORTED 256

const char* satrans_last_error(void);
int satrans_abi_version(void);

/* A non-blocking HIP stream of the LOWEST priority the current device offers, for work that must yield to the caller's launch
 * stream whenever both have a kernel ready (the engine's next-batch preparation; torch only hands out normal and higher).
 * SATRANS_E_UNSUPPORTED on a device with one priority level.  The caller owns the handle. */
int satrans_stream_create_low_priority(void** stream_out);
int satrans_stream_destroy(void* stream);

/* HOST function (no GPU involved): the sample order of a shuffled epoch, out[0..n) = the permutation torch.randperm(n, generator=g)
 * returns on the CPU for a generator seeded with `seed` - what the reference's DataLoader(shuffle=True) iterates over
 * (models/meta_basemodel.py:279-280 -> torch RandomSampler).  Same Fisher-Yates pass and Mersenne-Twister draws as torch, with the
 * swap partners drawn a block ahead and prefetched (several times faster than torch's 11-75 ns per row).  `progress` (optional):
 * receives, with release ordering, the count of leading positions that are final - a consumer on another thread may read
 * out[0..*progress) while the pass is still running.  SATRANS_E_UNSUPPORTED for n >= 2^32 / 20 (torch uses another algorithm there). */
int satrans_host_randperm(uint64_t seed, int64_t n, int64_t* out, int64_t* progress);

/* ------------------------------------------------------------------------------------------------
 * Scenario bucketing.  Reads the scenario id column of X (reference satrans.py:203:
 * `X[:, feature_index[domain_col][0]].long()`), writes
 *   sid[B]     scenario row per sample (clamped into [0,S) is NOT done: an id outside [0,S) sets
 *              status[0] = 1, the caller turns that into the IndexError the reference raises),
 *   order[B]   sample indices stably grouped by scenario,
 *   seg[S+1]   start of every scenario's run inside `order`.
 * x_stride = elements between consecutive samples of X; col = column of the scenario id.
 * ---------------------------------------------------------------------------------------------- */
int64_t satrans_bucket_workspace_bytes(int B, int S);
int satrans_bucket_scenarios(const void* X, int id_dtype, int64_t x_stride, int col, int B, int S,
                             int32_t* sid, int32_t* order, int32_t* seg, int32_t* status, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused multi-table embedding gather: reference meta_basemodel.py:533-535 (one nn.Embedding call per
 * SparseFeat) + concat_fun(axis=1) at satrans.py:211.
 *   arena      [total_rows, D] fp32: all tables back to back (any order; fields may share a table)
 *   row_span   [F][2] int64 (device): arena rows [lo, hi) of field f's table
 *   cols       [F] int32 (device): X column of field f
 *   out        [B, F, D]
 *   out        may be NULL: rows-only mode (ids -> arena rows, nothing is moved)
 *   rows_out   optional [B, F] int32: arena row of every gathered id (kept for the backward pass)
 *   status     [1] int32: set to 1 when an id falls outside its table
 * Bit-exact: every output element is a copy.
 * ---------------------------------------------------------------------------------------------- */
int satrans_gather_fwd(const float* arena, const int64_t* row_span, const int32_t* cols, const void* X,
                       int id_dtype, int64_t x_stride, int B, int F, int D, float* out,
                       int32_t* rows_out, int32_t* status, void* stream);
/* The grid of that launch, for a test that has to prove which of its loop trips it reaches: workgroups of SATRANS_GATHER_BLOCK
 * threads, D/4 lanes per row, SATRANS_GATHER_ROWS_PER_THREAD rows per thread and trip, enough workgroups for every row once
 * and never more than SATRANS_GATHER_MAX_BLOCKS (grid-strided beyond).  The pooled gather below is launched the same way
 * (SATRANS_POOL_ITEMS (sample, field) items per thread and trip; its backward takes one).  Not part of what a caller relies on. */
#define SATRANS_GATHER_BLOCK 256
#define SATRANS_GATHER_ROWS_PER_THREAD 4
#define SATRANS_GATHER_MAX_BLOCKS 2048
#define SATRANS_POOL_BLOCK 256
#define SATRANS_POOL_ITEMS 4
#define SATRANS_POOL_MAX_BLOCKS 2048

/* ------------------------------------------------------------------------------------------------
 * Pooled gather for models with VarLenSparseFeat fields: deepctr-torch's varlen_embedding_lookup + SequencePoolingLayer
 * behind the SparseFeat lookups, concatenated (reference meta_basemodel.py:519-545).  Field f occupies the `maxlen` SLOTS
 * [slot, slot + maxlen) of a sample; R = sum of maxlen over the fields (a SparseFeat is one slot with combiner COPY).
 *   fields     [F] HOST array, sparse fields first, then the varlen ones (F <= SATRANS_POOL_MAX_FIELDS; checked here and
 *              passed to the kernel by value).  slot / varlen must number the fields consecutively from 0.
 *   ids        X[b, col + s] (`.long()` truncation of fp32 ids); mask = s < X[b, len_col] when len_col >= 0, else id != 0
 *   SUM        sum over the valid slots in slot order (fp32)
 *   MEAN       the same sum / (count + 1e-8f), a true division; an empty list gives 0
 *   MAX        per element max over slots of (E - (1 - mask) * 1e9f); the first maximal slot wins.  An all-padding list
 *              gives about -1e9 (the reference's value)
 *   arena      [arena_rows, D]; an id outside [0, hi - lo) - padding slots included - sets bit 0 of *status, reads as zeros and
 *              is recorded as row lo
 *   src, src_rows  optional: the row of slot (b, r) is read from src + src_rows[b * R + r] * D instead of the arena (rows that
 *              arrived from their owners); rows_out is still computed from the ids
 *   out        [B, F, D] pooled layer input, or NULL (rows-only mode)
 *   rows_out   optional [B, R] int32 arena rows of every slot
 *   mask_out   [B, Fv] uint32: bit s = slot s of varlen field v is valid (needed with out when Fv > 0)
 *   argmax_out [B, Fv, D] uint8 (satrans_pool_argmax_bytes): slot of each MAX element (needed with out when Fv > 0)
 * Backward: dx [B, F, D] -> gemb [B * R, D], row b * R + r = gradient of slot r's row: COPY dx; SUM dx at valid slots, 0 at
 * padding; MEAN dx / (count + 1e-8f) at valid slots; MAX dx at the argmax slot of each element, 0 elsewhere.  Every element is
 * written exactly once (no atomics). */
#define SATRANS_POOL_COPY 0
#define SATRANS_POOL_SUM 1
#define SATRANS_POOL_MEAN 2
#define SATRANS_POOL_MAX 3
#define SATRANS_POOL_MAX_LEN 32
#define SATRANS_POOL_MAX_FIELDS 64
typedef struct satrans_pool_field {
    int32_t col;      /* first X column */
    int32_t maxlen;   /* 1 for a SparseFeat */
    int32_t combiner; /* SATRANS_POOL_* */
    int32_t len_col;  /* X column of the list length (length_name), or -1: mask = id != 0 */
    int32_t slot;     /* first slot in [0, R) */
    int32_t varlen;   /* index among the varlen fields, -1 for a SparseFeat */
    int64_t lo, hi;   /* arena rows [lo, hi) of the field's table */
} satrans_pool_field;
int64_t satrans_pool_argmax_bytes(int B, int Fv, int D);
int satrans_pool_gather_fwd(const float* arena, int64_t arena_rows, const float* src, const int32_t* src_rows,
                            const satrans_pool_field* fields, int F, int R, int Fv, const void* X, int id_dtype,
                            int64_t x_stride, int B, int D, float* out, int32_t* rows_out, uint32_t* mask_out,
                            uint8_t* argmax_out, int32_t* status, void* stream);
int satrans_pool_bwd(const float* dx, const satrans_pool_field* fields, int F, int R, int Fv, int B, int D,
                     const uint32_t* mask, const uint8_t* argmax, float* gemb, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The order-1 ("linear") term of deepctr's models: Linear.forward (reference models/meta_basemodel.py:63-92), the sum of 1-wide
 * embeddings of the sparse and (pooled) varlen fields plus dense @ weight, and its backward.  Added under ABI 7: new entry
 * points and a new struct type only.
 *   arena       [arena_rows] fp32: all 1-wide tables back to back
 *   fields      HOST array of F satrans_pool_field exactly as satrans_pool_gather_fwd takes it (sparse fields first, then the
 *               varlen ones; lo / hi are rows of the 1-wide arena; the same limits SATRANS_POOL_MAX_FIELDS / _MAX_LEN); F = 0
 *               (fields ignored, R = Fv = 0) leaves the dense term alone
 *   X, id_dtype, x_stride, B   as for the gather
 *   dense       the fp32 matrix the dense values are read from, rows dense_stride apart: X itself when X is fp32, the dense
 *               half of a packed input when the ids are integers
 *   dense_cols  [n_dense] int32 on the DEVICE: the column of `dense` of every dense value in concatenation order (a DenseFeat
 *               of dimension k is k columns); weight [n_dense]; both NULL with n_dense = 0.  A column outside
 *               [0, dense_stride) sets bit 1 of *status and reads as 0 (device values cannot be checked on the host).
 * F = 0 with n_dense = 0 is SATRANS_E_BADARG (nothing to compute: the caller returns zeros).
 *
 * satrans_linear_fwd:  logit[b] = sum_f pooled_f(b) + sum_k dense[b, dense_cols[k]] * weight[k]  in fp32 in THIS order: from
 * 0.0f the fields in descriptor order (the reference's sparse_embedding_list += varlen_embedding_list) by plain additions, then
 * k ascending by fmaf.  pooled_f follows the pooled gather's rules over 1-wide values: COPY w[row]; SUM over the valid slots in
 * slot order; MEAN that sum / (count + 1e-8f), a true division, an empty list 0; MAX the max over slots of w - (1 - mask) *
 * 1e9f, the first maximal slot winning; mask = s < X[b, len_col], or id != 0 with len_col < 0.  An id outside its table sets bit
 * 0 of *status, reads as 0 and is recorded as row lo.  A sample's logit does not depend on the batch around it: (sample,
 * field) items are spread over the lanes of a workgroup (SATRANS_LINEAR_SAMPLES samples per workgroup and trip, at most
 * SATRANS_LINEAR_MAX_BLOCKS workgroups, grid-strided beyond), the pooled values meet in LDS and one lane per sample adds them.
 *   logit [B, 1]; rows_out [B, R] int32; mask_out [B, Fv] uint32; argmax_out [B, Fv] uint8 (slot of the MAX value; 0 for the
 *   other combiners) - the last three needed with F > 0 (mask / argmax with Fv > 0)
 *
 * satrans_linear_bwd:  no floating-point atomics; the same call twice gives the same bits.
 *   contribution of slot position p = b R + r:  COPY dlogit[b]; SUM dlogit[b] at valid slots, 0 at padding; MEAN dlogit[b] /
 *     (count + 1e-8f) at valid slots; MAX dlogit[b] at the saved argmax slot, 0 elsewhere (materialised once, [B R] floats)
 *   g_arena[row] = the sum of its positions' contributions over (sorted_rows, src) = satrans_embed_sort(rows, n = B R,
 *     arena_rows, ...): the sorted list is cut into chunks of SATRANS_LINEAR_SEG_CHUNK positions at multiples of that number;
 *     inside a chunk a row's positions are added in position order; a row whose run crosses chunk bounds gets its per-chunk sums
 *     added in chunk order (one lane per such row).  The order depends on the sorted list alone, never on the grid.  The caller
 *     zero-fills g_arena: rows nobody gathered are not written.
 *   dweight[k] = sum_b dense[b, dense_cols[k]] * dlogit[b]: per SATRANS_LINEAR_DW_ROW_CHUNK rows a partial (fmaf, row order),
 *     the partials added in chunk order in fp64 (the heads' ordered reduce).  X gets no gradient.
 *   workspace: satrans_linear_workspace_bytes(d) bytes (negative: the error code of a bad descriptor).
 * All argument checks are made before a device is touched. */
#define SATRANS_LINEAR_SAMPLES 16
#define SATRANS_LINEAR_MAX_BLOCKS 512
#define SATRANS_LINEAR_SEG_CHUNK 32
#define SATRANS_LINEAR_DW_ROW_CHUNK 64
typedef struct satrans_linear_desc {
    int32_t B, F, R, Fv;
    int32_t id_dtype, n_dense;
    int64_t x_stride, arena_rows, dense_stride;
    const float* arena;
    const satrans_pool_field* fields;
    const void* X;
    const float* dense;
    const int32_t* dense_cols;
    const float* weight;
} satrans_linear_desc;
int64_t satrans_linear_workspace_bytes(const satrans_linear_desc* d);
int satrans_linear_fwd(const satrans_linear_desc* d, float* logit, int32_t* rows_out, uint32_t* mask_out, uint8_t* argmax_out,
                       int32_t* status, void* stream);
int satrans_linear_bwd(const satrans_linear_desc* d, const float* dlogit, const int32_t* rows, const uint32_t* mask,
                       const uint8_t* argmax, const int32_t* sorted_rows, const int32_t* src, float* g_arena, float* dweight,
                       void* workspace, void* stream);

/* Measurement aid (bench.py): the READ side of the gather alone - arena rows by row number (the `rows_out` of
 * satrans_gather_fwd), eight rows in flight per thread, nothing written but a checksum per thread into `sink`
 * (satrans_gather_read_probe_floats() floats).  This is the access pattern of the first layer with the gather fused in. */
int64_t satrans_gather_read_probe_floats(void);
int satrans_gather_read_probe(const float* arena, const int32_t* rows, int64_t n_rows, int D, float* sink, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-scenario generated weights (reference satrans.py:213,217-218; encoder = DNN_v2 with one Linear,
 * submodules.py:31-61): tab[s] = relu(emb[s]) @ W^T + bias for the S scenario rows (not per sample), and its backward.
 *   emb [S, De], W [P, De] (nn.Linear layout), bias [P], tab / g_tab [S, P]
 *   backward ADDS into g_emb [S, De], g_W [P, De], g_bias [P]; workspace: satrans_scenario_table_bwd_ws_floats floats
 * ---------------------------------------------------------------------------------------------- */
int satrans_scenario_table_fwd(const float* emb, const float* W, const float* bias, int S, int De, int P, float* tab,
                               void* stream);
int64_t satrans_scenario_table_bwd_ws_floats(int S, int De);
int satrans_scenario_table_bwd(const float* emb, const float* W, const float* g_tab, int S, int De, int P,
                               float* g_emb, float* g_W, float* g_bias, float* workspace, void* stream);

/* Encoder inputs of the variants (reference satrans.py:203-207 several scenario columns, :167-171,225-234 flag 'pos'):
 * row (lr * S + s) of E [LR * S, De], lr = 2 * layer + role (role 0 = Q, 1 = K; LR = 2 L with positions, else 1):
 *   E[.][0:D)  = mean over the C scenario columns of tables[c][index[c * S + s]]   (index == NULL: C = 1, row s itself)
 *   E[.][D:2D) = lay[layer] + role[role]                                           (lay / role given: De = 2 D)
 * The table kernels above then run on LR * S rows.  `tables` / `g_tables` / `table_rows` are HOST arrays of C entries
 * (device pointers / row counts), `index` is a device array [C, S].  The backward ADDS g_E (the g_emb output of
 * satrans_scenario_table_bwd) into g_tables[c] [rows_c, D], g_lay [L, D] and the first two rows of g_role, in a fixed order. */
int satrans_scenario_inputs_fwd(const float* const* tables, const int32_t* index, int C, int S, int D, const float* lay,
                                const float* role, int L, float* E, void* stream);
int satrans_scenario_inputs_bwd(float* const* g_tables, const int32_t* table_rows, const int32_t* index, int C, int S, int D,
                                const float* g_E, float* g_lay, float* g_role, int L, void* stream);
/* flag 'onlyemb' (satrans.py:173-176): tab = relu(emb) elementwise over n = S * P values; backward ADDS into g_emb */
int satrans_scenario_relu_fwd(const float* emb, int64_t n, float* tab, void* stream);
int satrans_scenario_relu_bwd(const float* emb, const float* g_tab, int64_t n, float* g_emb, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One Meta_Transformer_Layer (reference satrans.py:50-100 with MetaNet submodules.py:77-103).
 * The generated MetaNet weights are passed as per-scenario tables (one row per scenario id) instead
 * of the reference's per-sample [B,P] matrices; row s = encoder(relu(domain_embeddings[s])), see
 * satrans_amd/satrans.py.  tab_q / tab_k may alias (no 'pos' flag).
 * ---------------------------------------------------------------------------------------------- */
typedef struct satrans_layer_desc {
    int32_t B, F, D, H; /* batch, fields (tokens per sample), embedding dim, heads                   */
    int32_t U;          /* MetaNet hidden width; generated row = [D*U | U*D] (meta units [D,U,D])    */
    int32_t S;          /* scenario rows in tab_q / tab_k                                            */
    int32_t flags;      /* SATRANS_* bit mask                                                        */
    int32_t layer;      /* layer index, only used to key the dropout counters                        */
    float drop_p;       /* 0.1 in the reference (satrans.py:27-28)                                   */
    uint32_t seed, step;
    int64_t tab_stride; /* elements between scenario rows of tab_q / tab_k                           */
    const float* x;     /* [B,F,D] layer input                                                       */
    const int32_t* sid; /* [B]                                                                       */
    const int32_t* order; /* [B]  from satrans_bucket_scenarios                                      */
    const int32_t* seg;   /* [S+1]                                                                   */
    const float *w_query, *w_key, *w_value; /* [D,D], y = x @ W                                      */
    const float* w_out;                     /* [D,D] nn.Linear weight, y = x @ W^T                   */
    const float *ln_g, *ln_b;               /* layer_norm                                            */
    const float *lnq_g, *lnq_b, *lnk_g, *lnk_b; /* Q_/K_meta_mlp.ffn_layer_norm                      */
    const float *tab_q, *tab_k;             /* [S, >=P]                                              */
    const int32_t* x_rows; /* NULL, or [B,F] row numbers (the `rows` output of satrans_gather_fwd): the layer then   *
                            * reads token (b,f) from x + x_rows[b*F+f]*D, i.e. `x` is the embedding arena and the    *
                            * gather is fused into the first layer (meta_basemodel.py:533-535 + satrans.py:211 never *
                            * materialise [B,F,D]); forward and backward alike                                       */
    float* attn_save;      /* NULL, or satrans_layer_attn_save_floats(d) floats: the forward leaves what the backward  *
                            * would otherwise recompute (softmax numerators, 1 / sum, dropout keep word and the       *
                            * attention output, and - since late round 4, fp32 products - the normalised MetaNet rows  *
                            * of both roles with their 1 / std, all per SORTED sample position) and a satrans_layer_bwd *
                            * on the same batch, bucket order and dropout counters reads it instead of running its attention- *
                            * forward phase, the MetaNet's second products and its LayerNorm statistics.  The layout   *
                            * is the library's own: size it with satrans_layer_attn_save_floats, never by hand.        *
                            * Fused kernels only (others ignore it)                                                    */
} satrans_layer_desc;

/* Measurement aid (bench.py: `roofline.launch_ms`).  While armed (on != 0), every launch of the fused layer kernels is issued with a
 * pair of HIP events that the dispatch itself signals with its begin / end timestamps; satrans_kernel_timing_read waits for the
 * recorded launches, returns how many there were (<= max reported; at most 512 are kept between reads) with their kind - 0 layer
 * forward, 1 layer backward, 2 last layer + head in one launch (satrans_layer_bwd_head) - and duration in ms, and forgets them.
 * satrans_kernel_timing returns the previous state.  Process-wide, not thread-safe: for a single measuring thread. */
int satrans_kernel_timing(int on);
int satrans_kernel_timing_read(int* kinds, float* ms, int max);

/* Floats of `attn_save` for this layer (B samples), 0 when the kernels that would run it do not use one. */
int64_t satrans_layer_attn_save_floats(const satrans_layer_desc* d);

/* Which implementation evaluates satrans_layer_fwd/_bwd (process-wide; initial value from SATRANS_LAYER_IMPL):
 * 0 = automatic: register-chained f32-MFMA kernels for the shapes they are built for ((D,U,H) = (32,64,4), (16,32,2),
 *     (64,16,4)), else the LDS-resident kernels with MFMA products (D, U multiples of 16), else the same kernels
 *     with scalar FMA loops (any shape);
 * 1 = LDS-resident kernels with scalar FMA loops (the "wavefront/VALU" ablation arm);
 * 2 = LDS-resident kernels with MFMA products. */
int satrans_set_layer_impl(int impl);


/* 1 when the register-chained fused kernels (csrc/layer_fused.hip) are built for this layer: (D, H) = (32, 4) or (16, 2) with the
 * MetaNet width U = 2 D, or with SATRANS_GATE / SATRANS_BILINEAR (which replace the MetaNet: satrans.py:61-64,68-71,79-81);
 * forward only also (64, 4) with U = 16.  satrans_layer_fwd / _bwd pick them on their own; callers ask in order to choose
 * between this path and the general one (satrans_layer_generic_supported). */
int satrans_layer_fused_supported(const satrans_layer_desc* d);

/* Every product of the fused layer kernels (projections, MetaNet, Out_linear; satrans.py:55-57,60-73,91) runs on
 * v_mfma_f32_16x16x4_f32: bit for bit a chain of fmaf - what torch's CPU matmul computes up to summation order.  (ABI 4 had an
 * opt-in mode that split fp32 operands into bf16 pairs, satrans_set_product_mode; retired in ABI 5: outside the fp32 tolerance on
 * trained weights - tools/experiments/README.md.) */

/* y [B,F,D]; att optional [H,B,F,F] (`normalized_att_scores`, satrans.py:87) */
int satrans_layer_fwd(const satrans_layer_desc* d, float* y, float* att, void* stream);

/* Evaluation forward of one layer with the dense products on the bf16 matrix pipe (v_mfma_f32_16x16x32_bf16, fp32
 * accumulation; LayerNorm, softmax and the attention dot products in fp32; weights rounded to bf16 once per workgroup while
 * they are staged into LDS).  BASELINE.json configs[1] "bf16 forward": predict / evaluate only - no dropout (SATRANS_TRAIN
 * must be clear), no attention capture; results differ from satrans_layer_fwd by bf16 rounding (~1e-2 on the logits).
 * Built for
 *   - the MetaNet form (or no modulation) at (D,U,H) = (32,64,4) and (64,128,4), the latter for F <= 64;
 *   - SATRANS_GATE or SATRANS_BILINEAR at (D,H) = (32,4), any U (these flags have no MetaNet; U is ignored as in
 *     satrans_layer_fused_supported): gate scales q / k by 2 * the generated row in fp32 on the projection's accumulators,
 *     bilinear is one more bf16 product of q with the block-diagonal image of the H generated d x d maps;
 *   with the field count as a constant (matrix-pipe attention) for F = 19 and F = 15, at run time otherwise; one or two generated
 *   tables; x_rows.
 * Refused (_supported answers 0, the launch returns SATRANS_E_UNSUPPORTED): SATRANS_TRAIN, SATRANS_GATE together with
 * SATRANS_BILINEAR, either of them at any other (D,H) - (64,4) included: the general fp32 path serves it. */
int satrans_layer_fwd_bf16_supported(const satrans_layer_desc* d);
int satrans_layer_fwd_bf16(const satrans_layer_desc* d, float* y, void* stream);
/* The whole stack of n layers (satrans.py:236-239: `for layer in self.domain_int_layers`) of an EVALUATION forward as one launch: a
 * tile's rows stay in LDS between the layers - read from HBM once, written once - and every layer's weight images are staged once
 * per workgroup; per layer the code of satrans_layer_fwd_bf16, i.e. the same bits.  1 <= n <= 4 layers of D = 32 (every form
 * satrans_layer_fwd_bf16 is built for at D = 32: MetaNet, gate, bilinear) with one shape, one set of flags and one scenario bucketing; layer 0 reads its rows as satrans_layer_fwd_bf16 does (fused gather included), the
 * x / x_rows of the others are ignored.  y: the last layer's output [B][F][D]. */
int satrans_stack_fwd_bf16_supported(int n, const satrans_layer_desc* const* descs);
int satrans_stack_fwd_bf16(int n, const satrans_layer_desc* const* descs, float* y, void* stream);

/* General path for shapes the fused kernels are not built for (csrc/layer_generic.hip; first of all BASELINE configs[4]:
 * 64 fields, embedding_dim 64, MetaNet hidden 128): a layer as a short sequence of grouped f32-MFMA GEMM, LayerNorm and
 * attention launches over token rows kept in HBM in scenario-sorted order.  The forward SAVES its activations in `saved`
 * (satrans_layer_generic_saved_floats floats, one buffer per layer between forward and backward); the backward reads them and
 * uses `scratch` (satrans_layer_generic_scratch_floats floats, shared by all layers).  Arguments otherwise as
 * satrans_layer_fwd / satrans_layer_bwd (gradients ACCUMULATED in a fixed order; x_rows honoured).  Supported: D in
 * {16,32,64,128}, head dimension 8 or 16, U a multiple of 16 with D*U <= 8192; SATRANS_GATE or SATRANS_BILINEAR (not both):
 * the generated row is applied to q0 / k0 by an elementwise / per-head kernel, its gradient taken from the segment's z^T g.
 * satrans_set_generic_attention: attention arm of the forward - 0 automatic, 1 one lane per query row ("wavefront"),
 * 2 MFMA (F <= 64, head dimension 16), -1 back to SATRANS_GENERIC_ATTN / automatic. */
int satrans_layer_generic_supported(const satrans_layer_desc* d);
int64_t satrans_layer_generic_saved_floats(const satrans_layer_desc* d);
int64_t satrans_layer_generic_scratch_floats(const satrans_layer_desc* d);
int satrans_layer_fwd_generic(const satrans_layer_desc* d, float* y, float* att, float* saved, void* stream);
int satrans_layer_bwd_generic(const satrans_layer_desc* d, const float* dy, float* dx, const float* saved, float* scratch,
                              float* g_wq, float* g_wk, float* g_wv, float* g_wo, float* g_ln, float* g_lnq, float* g_lnk,
                              float* g_tab_q, float* g_tab_k, void* stream);
int satrans_set_generic_attention(int mode);

/* ------------------------------------------------------------------------------------------------
 * Sibling users of the same kernels, for the reference's baselines that plug the attention stack in.
 *
 * SelfAttention_Layer (models/submodules.py:178-238; `usetrans` in star.py, mmoe.py, ple.py, sharedbottom.py, adasparse.py):
 *     q,k,v = x W ; heads ; softmax(q k^T [/ sqrt(d)]) -> dropout -> @ v ; y = LayerNorm(relu(dropout(o) + x W_Res))
 * x, y, dy, dx [B,F,D] in the caller's order; W_* [D,D] (y = x @ W); g_ln [2,D] (gamma row, beta row).  Gradients are
 * ACCUMULATED (+=) in a fixed order; dx is written.  `saved` carries the forward's activations to the backward.
 * flags: SATRANS_TRAIN (dropout on), SATRANS_NO_RES (use_res=False), SATRANS_NO_SCALING (scaling=False). */
#define SATRANS_NO_SCALING 128
#define SATRANS_NO_NORM 256
typedef struct satrans_selfatt_desc {
    int32_t B, F, D, H, flags, layer;
    float drop_p;
    uint32_t seed, step;
    const float *x, *w_query, *w_key, *w_value, *w_res, *ln_g, *ln_b;
} satrans_selfatt_desc;
int64_t satrans_selfatt_saved_floats(const satrans_selfatt_desc* d);
int64_t satrans_selfatt_scratch_floats(const satrans_selfatt_desc* d);
int satrans_selfatt_fwd(const satrans_selfatt_desc* d, float* y, float* att, float* saved, void* stream);
int satrans_selfatt_bwd(const satrans_selfatt_desc* d, const float* dy, float* dx, const float* saved, float* scratch,
                        float* g_wq, float* g_wk, float* g_wv, float* g_wres, float* g_ln, void* stream);

/* MetaNet over an embedding block = BaseModel.meta_transformation (models/basemodel.py:191-199 with MetaNet,
 * models/submodules.py:64-103; `metatrans` in deepfm.py, dcn.py, ...):
 *     y = [LayerNorm](dropout(relu(x W1[s]) W2[s]) + x)      s = scenario of the sample, generated row tab[s] = [W1 D*U | W2 U*D]
 * order / seg from satrans_bucket_scenarios; flags: SATRANS_TRAIN, SATRANS_NO_NORM (MetaNet(use_norm=False)).
 * g_tab [S, tab_stride] and g_ln [2,D] are ACCUMULATED; dx is written. */
typedef struct satrans_metanet_desc {
    int32_t B, F, D, U, S, flags, layer;
    float drop_p;
    uint32_t seed, step;
    int64_t tab_stride;
    const float* x;
    const int32_t *order, *seg;
    const float *tab, *ln_g, *ln_b;
} satrans_metanet_desc;
int64_t satrans_metanet_saved_floats(const satrans_metanet_desc* d);
int64_t satrans_metanet_scratch_floats(const satrans_metanet_desc* d);
int satrans_metanet_fwd(const satrans_metanet_desc* d, float* y, float* saved, void* stream);
int satrans_metanet_bwd(const satrans_metanet_desc* d, const float* dy, float* dx, const float* saved, float* scratch,
                        float* g_tab, float* g_ln, void* stream);

/* Partitioned normalisation = one MDR_BatchNorm per scenario (models/submodules.py:107-175; the loop of star.py:147-154), all
 * scenarios in one pass:
 *     y[i] = (x[i] - mean[s]) * invstd[s] * (weight[s] * shared_w) + (bias[s] + shared_b)         s = scenario of row i
 * x, y, dy, dx [B,C] in the caller's row order; order / seg from satrans_bucket_scenarios; weight, bias, running_mean,
 * running_var [S,C]; shared_w, shared_b [C].
 * flags: SATRANS_TRAIN = normalise with the statistics of the batch (mean and biased variance over the scenario's rows) and,
 *     where running_mean / running_var are given, update them: r = (1 - factor) * r + factor * stat, the unbiased variance
 *     going into running_var.  Without it the running statistics normalise (both pointers required).
 * A scenario without rows leaves its running statistics untouched.  A scenario with ONE row has no unbiased variance: torch
 * refuses it, and so must the caller (the kernels then leave that scenario's running statistics untouched).
 * saved [2,S,C] = mean, invstd as used by the forward; the backward reads it.  The workspace holds the per-chunk partials of
 * the two-stage reductions (a chunk = SATRANS_PNORM_ROW_CHUNK rows of one scenario's run); the same buffer may serve both calls.
 * No floating-point atomics: every merge runs in a fixed order, the result depends on the inputs alone.
 * The backward WRITES dx, g_weight [S,C], g_bias [S,C], g_shared_w [C], g_shared_b [C] (not accumulated):
 *     training: dx = (g * invstd / n) * (n * dy - sum(dy) - xhat * sum(dy * xhat)),  g = weight[s] * shared_w,  sums over the scenario
 *     otherwise: dx = dy * g * invstd */
#define SATRANS_PNORM_ROW_CHUNK 128
typedef struct satrans_pnorm_desc {
    int32_t B, C, S, flags;
    float eps, factor;
    const float* x;
    const int32_t *order, *seg;
    const float *weight, *bias, *shared_w, *shared_b;
    float *running_mean, *running_var;
} satrans_pnorm_desc;
int64_t satrans_pnorm_saved_floats(const satrans_pnorm_desc* d);
int64_t satrans_pnorm_workspace_floats(const satrans_pnorm_desc* d);
int satrans_pnorm_fwd(const satrans_pnorm_desc* d, float* y, float* saved, float* workspace, void* stream);
int satrans_pnorm_bwd(const satrans_pnorm_desc* d, const float* dy, float* dx, const float* saved, float* workspace,
                      float* g_weight, float* g_bias, float* g_shared_w, float* g_shared_b, void* stream);

/* STAR's star-topology towers (models/star.py:156-170) for a mixed batch.  Layer l = 0 .. L-1 maps width n_{l-1} to n_l = width[l]
 * (n_{-1} = C; the last layer is the logit, width[L-1] == 1); row i belongs to scenario s:
 *     W_eff[s,l] = w_dom[l][s] * w_sh[l]   (elementwise, [n_l, n_{l-1}])        b_eff[s,l] = b_dom[l][s] + b_sh[l]
 *     h_l[i] = relu(h_{l-1}[i] W_eff[s,l]^T + b_eff[s,l])   for l < L-1,        logit[i] = h_{L-2}[i] W_eff[s,L-1]^T + b_eff[s,L-1]
 * x [B,C], logit / dlogit [B] and dx [B,C] in the caller's row order; order / seg from satrans_bucket_scenarios;
 * w_dom[l] [S, n_l, n_{l-1}], b_dom[l] [S, n_l] (the scenarios' parameters stacked), w_sh[l] [n_l, n_{l-1}], b_sh[l] [n_l].
 * fp32 throughout, products on the exact f32-input MFMA.  C and the widths are any positive integers; 1 to 4 hidden layers.
 * saved = the hidden rows h_0 .. h_{L-2}, [B, n_l] each, layer after layer, in the caller's row order: B * sum of the hidden
 * widths floats; the backward reads them (nothing is recomputed).  The forward needs no workspace; the backward's holds two
 * [B, widest hidden layer] buffers for dz and the per-chunk partials of the weight gradients of the layer in hand
 * (a chunk = SATRANS_STAR_DW_ROW_CHUNK rows counted from the start of a scenario's run):
 *     2 * B * max hidden width + (ceil(B / SATRANS_STAR_DW_ROW_CHUNK) + S) * max over l of n_l * (n_{l-1} + 1)   floats.
 * The backward WRITES (does not accumulate) dx and, per layer, g_w_dom[l] [S, n_l, n_{l-1}], g_b_dom[l] [S, n_l],
 * g_w_sh[l] [n_l, n_{l-1}], g_b_sh[l] [n_l] (arrays of L pointers):
 *     dz_l = dh_l * (h_l > 0)  (dz_{L-1} = dlogit),   dh_{l-1} = dz_l W_eff[s,l],   dW_eff[s,l] = dz_l^T h_{l-1} over the scenario's rows,
 *     g_w_dom = dW_eff * w_sh,  g_b_dom = column sums of dz_l,  g_w_sh = sum over s of dW_eff[s] * w_dom[s],  g_b_sh = sum over s of g_b_dom[s].
 * No floating-point atomics: chunks merge in chunk order, scenarios in scenario order, so equal inputs give equal bits and a
 * scenario's rows give the same bits alone as inside a mixed batch.  A scenario without rows gets zeros in its gradients. */
#define SATRANS_STAR_ROW_TILE 64
#define SATRANS_STAR_DW_ROW_CHUNK 256
#define SATRANS_STAR_MAX_LAYERS 5
typedef struct satrans_star_desc {
    int32_t B, C, S, L;
    int32_t width[SATRANS_STAR_MAX_LAYERS];
    int32_t reserved;      /* 0 */
    const float* x;
    const int32_t *order, *seg;
    const float* w_dom[SATRANS_STAR_MAX_LAYERS];
    const float* b_dom[SATRANS_STAR_MAX_LAYERS];
    const float* w_sh[SATRANS_STAR_MAX_LAYERS];
    const float* b_sh[SATRANS_STAR_MAX_LAYERS];
} satrans_star_desc;
int64_t satrans_star_saved_floats(const satrans_star_desc* d);
int64_t satrans_star_workspace_floats(const satrans_star_desc* d);
int satrans_star_fwd(const satrans_star_desc* d, float* logit, float* saved, void* stream);
int satrans_star_bwd(const satrans_star_desc* d, const float* dlogit, float* dx, const float* saved, float* workspace,
                     float* const* g_w_dom, float* const* g_b_dom, float* const* g_w_sh, float* const* g_b_sh, void* stream);

/* Scenario-routed MMoE head (models/mmoe.py:142-171 under the per-scenario loss of mtl_basemodel.py:268-269) for a mixed batch:
 * the E experts run over all rows, and row i of scenario (= task) t goes through task t's gate, mixture, tower and logit only.
 *     experts   h^e_l = relu(h^e_{l-1} expert_w[l][e]^T + expert_b[l][e]),  h^e_0 = x,  l = 1 .. n_expert;  expert_out[e] = h^e_{n_expert}
 *     gate      the DNN gate_w[l][t] / gate_b[l][t] (relu) over x, then scores = h gate_final_w[t]^T  [E]   (n_gate = 0: over x)
 *     mixture   g = softmax(scores),  m = sum_e g[e] expert_out[e]
 *     tower     the DNN tower_w[l][t] / tower_b[l][t] (relu) over m, then logit = h tower_final_w[t]^T + out_bias[t]
 * x [B,C], logit / dlogit [B] and dx [B,C] in the caller's row order; order / seg from satrans_bucket_scenarios with S = T.
 * Stacked parameters: expert_w[l] [E, n_l, n_{l-1}], expert_b[l] [E, n_l]; gate_w[l] [T, n_l, n_{l-1}], gate_b[l] [T, n_l],
 * gate_final_w [T, E, n]; tower_w[l], tower_b[l] likewise, tower_final_w [T, 1, n], out_bias [T].
 * fp32 throughout, products on the exact f32-input MFMA.  2 <= E <= SATRANS_MMOE_MAX_EXPERTS; 1 to SATRANS_MMOE_MAX_HIDDEN
 * expert layers, 0 to SATRANS_MMOE_MAX_HIDDEN gate and tower layers; C and the widths are any positive integers.
 * saved, from its start: the gates g [B,E], the mixture m [B, n of the last expert layer], the scores [B,E], then every hidden
 * row in the caller's row order (experts [B, E n_l] with expert e in columns [e n_l, (e+1) n_l), gate, tower); the backward
 * reads them (nothing is recomputed).  The forward needs no workspace; the backward's holds two [B, widest row] dz buffers,
 * dscores [B,E] and the per-chunk partials of the weight gradients of the layer in hand (a chunk =
 * SATRANS_MMOE_DW_ROW_CHUNK rows: counted from the start of a task's run for gate and tower, in the caller's row order for
 * the experts).  The backward WRITES (does not accumulate) dx and every gradient of satrans_mmoe_grads, each of the shape of
 * its parameter.  No floating-point atomics: chunks merge in chunk order, dx = experts' dx + gate's dx in that order, so equal
 * inputs give equal bits and a task's rows give the same bits alone as inside a mixed batch (logit, dx, that task's gate,
 * tower and out_bias gradients).  A task without rows gets zeros in its gradients. */
#define SATRANS_MMOE_ROW_TILE 64
#define SATRANS_MMOE_DW_ROW_CHUNK 256
#define SATRANS_MMOE_MAX_EXPERTS 8
#define SATRANS_MMOE_MAX_HIDDEN 3
typedef struct satrans_mmoe_desc {
    int32_t B, C, T, E;
    int32_t n_expert, n_gate, n_tower;      /* hidden layers of the three DNNs */
    int32_t reserved;                       /* 0 */
    int32_t expert_width[SATRANS_MMOE_MAX_HIDDEN];
    int32_t gate_width[SATRANS_MMOE_MAX_HIDDEN];
    int32_t tower_width[SATRANS_MMOE_MAX_HIDDEN];
    int32_t reserved2;                      /* 0 */
    const float* x;
    const int32_t *order, *seg;
    const float* expert_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* expert_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* gate_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* gate_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* gate_final_w;
    const float* tower_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* tower_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* tower_final_w;
    const float* out_bias;
} satrans_mmoe_desc;
typedef struct satrans_mmoe_grads {
    float* expert_w[SATRANS_MMOE_MAX_HIDDEN];
    float* expert_b[SATRANS_MMOE_MAX_HIDDEN];
    float* gate_w[SATRANS_MMOE_MAX_HIDDEN];
    float* gate_b[SATRANS_MMOE_MAX_HIDDEN];
    float* gate_final_w;
    float* tower_w[SATRANS_MMOE_MAX_HIDDEN];
    float* tower_b[SATRANS_MMOE_MAX_HIDDEN];
    float* tower_final_w;
    float* out_bias;
} satrans_mmoe_grads;
int64_t satrans_mmoe_saved_floats(const satrans_mmoe_desc* d);
int64_t satrans_mmoe_workspace_floats(const satrans_mmoe_desc* d);
int satrans_mmoe_fwd(const satrans_mmoe_desc* d, float* logit, float* saved, void* stream);
int satrans_mmoe_bwd(const satrans_mmoe_desc* d, const float* dlogit, float* dx, const float* saved, float* workspace,
                     const satrans_mmoe_grads* g, void* stream);

/* Scenario-routed PLE head (models/ple.py:161-248 under the per-scenario loss of mtl_basemodel.py:268-269) for a mixed batch,
 * one or two CGC levels.  T tasks, ns specific experts per task, nsh shared experts; every expert is the relu DNN of widths
 * expert_width, every gate the relu DNN of widths gate_width and a bias-free final layer.  Row i of task t = task[i]:
 *   level 0 of two (dense unless stated): all E0 = T ns + nsh experts over x (blocks: task 0's ns, task 1's, ..., the shared);
 *     own gate g0 (ROUTED: task t's) -> softmax over t's ns experts then the nsh shared ones -> own mixture;
 *     shared gate sg0 -> softmax over all E0 blocks ascending -> shared mixture.
 *   last level: task t's ns specific experts over the own mixture (ROUTED; over x with one level), the nsh shared experts over
 *     the shared mixture (dense; over x with one level), task t's gate over the own mixture -> softmax over [specific, shared]
 *     -> mixture -> task t's tower, tower_final_w and out_bias -> logit.  The last level's shared gate takes no part.
 * Stacked parameters: e0_w[l] [E0, n_l, n_{l-1}], e0_b[l] [E0, n_l]; g0_w[l] [T, n_l, n_{l-1}], g0_b[l] [T, n_l], g0_final_w
 * [T, ns + nsh, n]; sg0_w[l] [n_l, n_{l-1}], sg0_b[l] [n_l], sg0_final_w [E0, n]; spec_w[l] [T, ns, n_l, n_{l-1}], spec_b[l]
 * [T, ns, n_l]; shared_w[l] [nsh, n_l, n_{l-1}], shared_b[l] [nsh, n_l]; gate_*, tower_*, out_bias as in satrans_mmoe_desc with
 * E = ns + nsh.  With levels == 1 the e0 / g0 / sg0 fields and `task` are not read.
 * x [B,C], logit / dlogit [B], dx [B,C], task [B] (int32, the row's task) in the caller's row order; order / seg from
 * satrans_bucket_scenarios with S = T.  fp32 throughout, the products of the MMoE head (one more form: routed AND grouped
 * within the task).  Limits: levels 1 or 2; nsh >= 1, ns >= 1, ns + nsh <= SATRANS_PLE_MAX_OWN; T ns + nsh <=
 * SATRANS_PLE_MAX_SHARED_SCORES; 1 to SATRANS_PLE_MAX_HIDDEN expert layers, 0 to SATRANS_PLE_MAX_HIDDEN gate and tower layers.
 * saved, from its start: the last level's gates [B, ns + nsh], mixture [B, n], scores, its hidden rows ([B, (ns + nsh) n_l]:
 * the task's specific experts, then the shared ones), gate and tower rows; then, with two levels, own gates [B, ns + nsh],
 * shared gates [B, E0], own mixture, shared mixture, both scores, level 0's hidden rows [B, E0 n_l] and both gates' rows.
 * Nothing is recomputed.  The backward WRITES dx and every gradient of satrans_ple_grads.  No floating-point atomics; fixed
 * orders: dx = level-0 experts' dx, + own gate's, + shared gate's (one level: specific experts', + shared experts', + gate's);
 * d own mixture = specific experts' dx, + last-level gate's dx.  Equal inputs give equal bits; a task's rows give the same bits
 * alone as inside a mix (logit, dx rows, the task's gates, last-level experts, tower, out_bias); the dense gradients sum
 * over all rows in the caller's order (chunks of SATRANS_PLE_DW_ROW_CHUNK rows).  A task without rows gets zeros in its routed
 * gradients. */
#define SATRANS_PLE_ROW_TILE 64
#define SATRANS_PLE_DW_ROW_CHUNK 256
#define SATRANS_PLE_MAX_OWN 8
#define SATRANS_PLE_MAX_SHARED_SCORES 64
#define SATRANS_PLE_MAX_HIDDEN 3
typedef struct satrans_ple_desc {
    int32_t B, C, T, ns, nsh, levels;
    int32_t n_expert, n_gate, n_tower;      /* hidden layers of the three kinds of DNN */
    int32_t reserved;                       /* 0 */
    int32_t expert_width[SATRANS_PLE_MAX_HIDDEN];
    int32_t gate_width[SATRANS_PLE_MAX_HIDDEN];
    int32_t tower_width[SATRANS_PLE_MAX_HIDDEN];
    int32_t reserved2;                      /* 0 */
    const float* x;
    const int32_t *order, *seg, *task;
    const float* e0_w[SATRANS_PLE_MAX_HIDDEN];
    const float* e0_b[SATRANS_PLE_MAX_HIDDEN];
    const float* g0_w[SATRANS_PLE_MAX_HIDDEN];
    const float* g0_b[SATRANS_PLE_MAX_HIDDEN];
    const float* g0_final_w;
    const float* sg0_w[SATRANS_PLE_MAX_HIDDEN];
    const float* sg0_b[SATRANS_PLE_MAX_HIDDEN];
    const float* sg0_final_w;
    const float* spec_w[SATRANS_PLE_MAX_HIDDEN];
    const float* spec_b[SATRANS_PLE_MAX_HIDDEN];
    const float* shared_w[SATRANS_PLE_MAX_HIDDEN];
    const float* shared_b[SATRANS_PLE_MAX_HIDDEN];
    const float* gate_w[SATRANS_PLE_MAX_HIDDEN];
    const float* gate_b[SATRANS_PLE_MAX_HIDDEN];
    const float* gate_final_w;
    const float* tower_w[SATRANS_PLE_MAX_HIDDEN];
    const float* tower_b[SATRANS_PLE_MAX_HIDDEN];
    const float* tower_final_w;
    const float* out_bias;
} satrans_ple_desc;
typedef struct satrans_ple_grads {
    float* e0_w[SATRANS_PLE_MAX_HIDDEN];
    float* e0_b[SATRANS_PLE_MAX_HIDDEN];
    float* g0_w[SATRANS_PLE_MAX_HIDDEN];
    float* g0_b[SATRANS_PLE_MAX_HIDDEN];
    float* g0_final_w;
    float* sg0_w[SATRANS_PLE_MAX_HIDDEN];
    float* sg0_b[SATRANS_PLE_MAX_HIDDEN];
    float* sg0_final_w;
    float* spec_w[SATRANS_PLE_MAX_HIDDEN];
    float* spec_b[SATRANS_PLE_MAX_HIDDEN];
    float* shared_w[SATRANS_PLE_MAX_HIDDEN];
    float* shared_b[SATRANS_PLE_MAX_HIDDEN];
    float* gate_w[SATRANS_PLE_MAX_HIDDEN];
    float* gate_b[SATRANS_PLE_MAX_HIDDEN];
    float* gate_final_w;
    float* tower_w[SATRANS_PLE_MAX_HIDDEN];
    float* tower_b[SATRANS_PLE_MAX_HIDDEN];
    float* tower_final_w;
    float* out_bias;
} satrans_ple_grads;
int64_t satrans_ple_saved_floats(const satrans_ple_desc* d);
int64_t satrans_ple_workspace_floats(const satrans_ple_desc* d);
int satrans_ple_fwd(const satrans_ple_desc* d, float* logit, float* saved, void* stream);
int satrans_ple_bwd(const satrans_ple_desc* d, const float* dlogit, float* dx, const float* saved, float* workspace,
                    const satrans_ple_grads* g, void* stream);

/* AdaSparse's scenario-pruned DNN (models/adasparse.py:88-106 with use_bn = False, relu, no dropout) and the bias-free logit
 * layer behind it (adasparse.py:185-189).  Nothing is routed: every row uses the same weights, and the scenario enters through
 * the row's scenario embedding emb [B,E] only.  Layer l = 1 .. n_layers, h_0 = x [B,C], K = n_{l-1}, N = n_l = width[l-1]:
 *     fc  = h_{l-1} lin_w[l]^T + lin_b[l]                      lin_w[l] [N, K],     lin_b[l] [N]
 *     z   = [h_{l-1} | emb] prn_w[l]^T + prn_b[l]              prn_w[l] [N, K + E], prn_b[l] [N]
 *     pi  = beta * sigmoid(alpha * z),  pi = 0 where |pi| - epsilon <= 0
 *     h_l = relu(fc * pi)
 *     logit = h_L final_w^T + out_bias[0]                      final_w [1, n_L], out_bias [1]
 * fp32 throughout, products on the exact f32-input MFMA; the concatenation [h | emb] is never materialised (the forward
 * layer is ONE launch: both products over one staged row tile, then the epilogue).  1 to SATRANS_MMOE_MAX_HIDDEN layers; C,
 * E and the widths are any positive integers; beta > 0, epsilon >= 0.
 * saved, from its start, per layer l: pi [B, n_l] (the pruned factors), dzf = fc alpha pi (1 - pi / beta) [B, n_l] (the forward
 * forms 1 - pi / beta = sigmoid(-alpha z) from z, where it keeps its digits), h_l [B, n_l]; the backward reads them.  The forward needs no workspace.  The backward's holds two [B, widest layer] buffers
 * of masked output gradients, [dfc | dz] [B, 2 widest layer] and the per-chunk partials of the weight gradients of the layer
 * in hand (a chunk = SATRANS_MMOE_DW_ROW_CHUNK rows in the caller's row order).  With g = dh_l (fc pi > 0):
 *     dfc = g pi,   dz = g dzf (exactly 0 where pruned),
 *     dh_{l-1} = dfc lin_w[l] + dz prn_w[l][:, :K],   demb += dz prn_w[l][:, K:]  (last layer first),
 *     d lin_w[l] = dfc^T h_{l-1},  d prn_w[l] = dz^T [h_{l-1} | emb],  d lin_b[l], d prn_b[l] = the column sums.
 * The backward WRITES (does not accumulate) dx [B,C], demb [B,E] and every gradient of satrans_adasparse_grads, each of the
 * shape of its parameter.  No floating-point atomics: chunks merge in chunk order and demb sums the layers last to first, so
 * equal inputs give equal bits, and a row gives the same logit, dx and demb bits alone as inside any batch.
 * final_w and out_bias both NULL: the DNN alone - no logit is written (h_L is the last [B, n_L] block of saved), the backward's
 * `dlogit` is then dh_L [B, n_L] (put under h_L's relu mask there) and the two gradients of satrans_adasparse_grads are not written.
 * satrans_adasparse_set_forward(1) makes the forward run each layer as two launches of the plain tile product (the second over
 * a concatenated copy of [h | emb], kept behind the saved rows) and a pointwise kernel - the form the fused launch was measured
 * against (tools/adasparse_time.py); 0, the default, is the fused launch.  Process-wide; the same mode must hold for the
 * saved_floats call and the forward it sizes.  Returns the previous mode, or SATRANS_E_BADARG. */
typedef struct satrans_adasparse_desc {
    int32_t B, C, E, n_layers;
    int32_t width[SATRANS_MMOE_MAX_HIDDEN];
    float alpha, beta, epsilon;
    const float *x, *emb;
    const float* lin_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* lin_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* prn_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* prn_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* final_w;
    const float* out_bias;
} satrans_adasparse_desc;
typedef struct satrans_adasparse_grads {
    float* lin_w[SATRANS_MMOE_MAX_HIDDEN];
    float* lin_b[SATRANS_MMOE_MAX_HIDDEN];
    float* prn_w[SATRANS_MMOE_MAX_HIDDEN];
    float* prn_b[SATRANS_MMOE_MAX_HIDDEN];
    float* final_w;
    float* out_bias;
} satrans_adasparse_grads;
int64_t satrans_adasparse_saved_floats(const satrans_adasparse_desc* d);
int64_t satrans_adasparse_workspace_floats(const satrans_adasparse_desc* d);
int satrans_adasparse_fwd(const satrans_adasparse_desc* d, float* logit, float* saved, void* stream);
int satrans_adasparse_bwd(const satrans_adasparse_desc* d, const float* dlogit, float* dx, float* demb, const float* saved,
                          float* workspace, const satrans_adasparse_grads* g, void* stream);
int satrans_adasparse_set_forward(int composed);

/* Scenario-routed SharedBottom head (models/sharedbottom.py:120-133 under the per-scenario loss of mtl_basemodel.py:268-269)
 * for a mixed batch: the bottom DNN runs over all rows, and row i of scenario (= task) t goes through task t's tower only.
 *     bottom    h_l = relu(h_{l-1} bottom_w[l]^T + bottom_b[l]),  h_0 = x,  l = 1 .. n_bottom                      (all rows)
 *     tower     the DNN tower_w[l][t] / tower_b[l][t] (relu) over the bottom's last rows, then
 *               logit = h tower_final_w[t]^T + out_bias[t]                       (n_tower = 0: over the bottom's last rows)
 * x [B,C], logit / dlogit [B] and dx [B,C] in the caller's row order; order / seg from satrans_bucket_scenarios with S = T.
 * bottom_w[l] [n_l, n_{l-1}], bottom_b[l] [n_l]; tower_w[l] [T, n_l, n_{l-1}], tower_b[l] [T, n_l], tower_final_w [T, 1, n],
 * out_bias [T].  fp32 throughout, products on the exact f32-input MFMA.  1 to SATRANS_MMOE_MAX_HIDDEN bottom layers, 0 to
 * SATRANS_MMOE_MAX_HIDDEN tower layers; C and the widths are any positive integers.  Row tiles and weight-gradient chunks are
 * those of the MMoE head (SATRANS_MMOE_ROW_TILE, SATRANS_MMOE_DW_ROW_CHUNK).
 * The tower tail - the last tower layer, the final layer and out_bias - is ONE launch: a workgroup takes a row tile of a
 * task's run, walks the 64-column tiles of the last tower layer, writes h = relu(acc + b) to saved and continues per row the
 * chain logit = fmaf(h[n], tower_final_w[t][n], logit), n ascending from 0 over all tiles; logit + out_bias[t] is written.
 * That is the arithmetic order of the tile product with one output column followed by its bias.  With n_tower = 0 the tail is
 * the row-wise chain over the bottom's last rows.  satrans_sharedbottom_set_forward(1) makes the forward run the tail as those
 * tile products instead (two launches, one with n_tower = 0), the form the tail was measured against
 * (tools/sharedbottom_time.py): same bits in logit and saved.  0 is the fused tail.  Process-wide; returns the previous mode,
 * or SATRANS_E_BADARG.
 * saved: every hidden row in the caller's row order, the bottom's layers [B, n_l] first, then the tower's; the backward reads
 * them.  The forward needs no workspace; the backward's holds two [B, widest row] dz buffers and the per-chunk partials of the
 * weight gradients of the layer in hand (chunks counted from the start of a task's run for the towers, in the caller's row
 * order for the bottom).  The tail's backward is pointwise, dz[row, n] = dlogit[row] tower_final_w[t][n] (h[row, n] > 0), and
 * forms the chunk partials of d tower_final_w and d out_bias in the same pass.  The backward WRITES (does not accumulate) dx
 * and every gradient of satrans_sharedbottom_grads, each of the shape of its parameter.  No floating-point atomics: chunks
 * merge in chunk order, so equal inputs give equal bits and a task's rows give the same bits alone as inside a mixed batch
 * (logit, dx, that task's tower, final-layer and out_bias gradients).  A task without rows gets zeros in its gradients. */
typedef struct satrans_sharedbottom_desc {
    int32_t B, C, T;
    int32_t n_bottom, n_tower;              /* hidden layers of the two DNNs */
    int32_t reserved;                       /* 0 */
    int32_t bottom_width[SATRANS_MMOE_MAX_HIDDEN];
    int32_t tower_width[SATRANS_MMOE_MAX_HIDDEN];
    const float* x;
    const int32_t *order, *seg;
    const float* bottom_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* bottom_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* tower_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* tower_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* tower_final_w;
    const float* out_bias;
} satrans_sharedbottom_desc;
typedef struct satrans_sharedbottom_grads {
    float* bottom_w[SATRANS_MMOE_MAX_HIDDEN];
    float* bottom_b[SATRANS_MMOE_MAX_HIDDEN];
    float* tower_w[SATRANS_MMOE_MAX_HIDDEN];
    float* tower_b[SATRANS_MMOE_MAX_HIDDEN];
    float* tower_final_w;
    float* out_bias;
} satrans_sharedbottom_grads;
int64_t satrans_sharedbottom_saved_floats(const satrans_sharedbottom_desc* d);
int64_t satrans_sharedbottom_workspace_floats(const satrans_sharedbottom_desc* d);
int satrans_sharedbottom_fwd(const satrans_sharedbottom_desc* d, float* logit, float* saved, void* stream);
int satrans_sharedbottom_bwd(const satrans_sharedbottom_desc* d, const float* dlogit, float* dx, const float* saved,
                             float* workspace, const satrans_sharedbottom_grads* g, void* stream);
int satrans_sharedbottom_set_forward(int composed);

/* Compressed interaction network: deepctr-torch's CIN, the interaction layer of the reference's xDeepFM (models/xdeepfm.py:73,
 * 96-98).  With X0 = x0 [B, M, D], H_0 = M and X_0 = X0, layer i = 0 .. L-1 of O_i = width[i] channels:
 *     z_i[b,o,d] = b[i][o] + sum_{h < H_i, m < M} w[i][o, h M + m] X_i[b,h,d] X0[b,m,d]        a_i = relu(z_i)
 *     split_half and i < L-1:  X_{i+1} = a_i[:, :O_i/2], direct_i = a_i[:, O_i/2:]   (O_i even, else SATRANS_E_BADARG)
 *     otherwise:               X_{i+1} = direct_i = a_i
 *     result [B, F] = the direct channels of layer 0, then layer 1, ..., each summed over d (d ascending)
 * w[i] [O_i, H_i M] (the Conv1d(H_i M, O_i, 1) weight without its last axis), b[i] [O_i].  fp32 throughout, products on the
 * exact f32-input MFMA.  1 to SATRANS_CIN_MAX_LAYERS layers, 1 to SATRANS_CIN_MAX_FIELDS fields, widths 1 to
 * SATRANS_CIN_MAX_WIDTH, any positive B and D with B D < 2^31 (SATRANS_E_UNSUPPORTED beyond).
 * The outer product [B, H_i M, D] of the torch form is never written: a product's rows are the (b, d) pairs r = b D + d, its
 * contraction index is k = h M + m, and the operand element X_i[b,h,d] X0[b,m,d] is formed from two values in LDS while w[i]
 * streams.  A workgroup takes SATRANS_CIN_ROW_TILE rows r; a result element is a k-ordered fmaf chain, so a sample's row of
 * `result` does not depend on the batch around it.
 * saved: a_i [B, O_i, D] of every layer, layer 0 first - all the backward keeps.  The forward needs no workspace; the
 * backward's holds dz [B, widest layer, D], dX of the layer above [B, widest hidden part, D] and the per-chunk partials of
 * the weight gradients of the layer in hand (a chunk = SATRANS_CIN_DW_ROW_CHUNK rows r).  Per layer, last to first:
 * dz = upstream (a_i > 0); dw[i] = dz^T A and db[i] = sum dz as chunk partials, the operand generated again, merged in chunk
 * order; dA = dz w[i] is never stored - the workgroup of a row tile walks the tiles of k in order and folds each into
 * dX_i[b,h,d] += dA X0[b,m,d] and dX0[b,m,d] += dA X_i[b,h,d] (layer 0: both into dX0).  The backward WRITES dx0 [B, M, D]
 * and every gradient of satrans_cin_grads.  No floating-point atomics: equal inputs give equal bits, and a sample's dx0 rows
 * are the same bits alone as inside a batch. */
#define SATRANS_CIN_MAX_LAYERS 4
#define SATRANS_CIN_MAX_FIELDS 64
#define SATRANS_CIN_MAX_WIDTH 256
#define SATRANS_CIN_ROW_TILE 64
#define SATRANS_CIN_DW_ROW_CHUNK 1024
typedef struct satrans_cin_desc {
    int32_t B, M, D, L;
    int32_t split_half;                     /* 0 or 1 */
    int32_t reserved;                       /* 0 */
    int32_t width[SATRANS_CIN_MAX_LAYERS];
    const float* x0;
    const float* w[SATRANS_CIN_MAX_LAYERS];
    const float* b[SATRANS_CIN_MAX_LAYERS];
} satrans_cin_desc;
typedef struct satrans_cin_grads {
    float* w[SATRANS_CIN_MAX_LAYERS];
    float* b[SATRANS_CIN_MAX_LAYERS];
} satrans_cin_grads;
int64_t satrans_cin_saved_floats(const satrans_cin_desc* d);
int64_t satrans_cin_workspace_floats(const satrans_cin_desc* d);
int satrans_cin_fwd(const satrans_cin_desc* d, float* result, float* saved, void* stream);
int satrans_cin_bwd(const satrans_cin_desc* d, const float* dresult, float* dx0, const float* saved, float* workspace,
                    const satrans_cin_grads* g, void* stream);

/* DCN's cross network: deepctr-torch's CrossNet, which the reference's DCN calls (models/dcn.py:70,101), in its vector
 * (matrix = 0) and matrix (matrix = 1) forms.  With x0 [B, N], x_0 = x0, l = 0 .. L-1:
 *     vector:  s_l[b]   = sum_n x_l[b,n] kernels[l][n]          x_{l+1} = x0 s_l[b] + bias[l] + x_l
 *     matrix:  u_l[b,:] = kernels[l] x_l[b,:] + bias[l]         x_{l+1} = x0 * u_l + x_l       (kernels[l] [n_out, n_in])
 *     result [B, N] = x_L
 * kernels [L, N] (deepctr's [L, N, 1]) or [L, N, N], bias [L, N] (deepctr's [L, N, 1]).  fp32 throughout.  1 to
 * SATRANS_CROSS_MAX_LAYERS layers, 1 to SATRANS_CROSS_MAX_FEATURES features, any positive B whose launches fit 2^31
 * workgroups (SATRANS_E_UNSUPPORTED beyond); all of that is decided before a device is touched.
 * Vector form: one launch forward (a wave per row, the row in registers over all layers; x0 read once, result written once)
 * and one backward launch plus the ordered reduce.  saved = s [B, L]: B L floats.  The backward rebuilds x_l from x0 and s
 * (x_l = (1 + sum_{j<l} s_j) x0 + sum_{j<l} bias[j]); a workgroup owns SATRANS_CROSS_VEC_ROW_CHUNK rows and leaves one partial
 * of dkernels and dbias: workspace = 2 ceil(B / SATRANS_CROSS_VEC_ROW_CHUNK) L N floats.
 * Matrix form: one launch per layer forward, the 64 x 64 f32-MFMA tile product with the cross epilogue.
 * saved = u_0 .. u_{L-1} [B, N] each, then x_1 .. x_{L-1}: (2 L - 1) B N floats.  workspace = du [B, N], g [B, N] and the
 * partials of one layer's dkernels and dbias, ceil(B / SATRANS_MMOE_DW_ROW_CHUNK) N (N + 1): 2 B N + that, floats.
 * The backward WRITES dx [B, N] and both gradients.  No floating-point atomics: equal inputs give equal bits, and a sample's
 * result row and dx row are the same bits alone as inside a batch. */
#define SATRANS_CROSS_MAX_LAYERS 8
#define SATRANS_CROSS_MAX_FEATURES 4096
#define SATRANS_CROSS_VEC_ROW_CHUNK 32
typedef struct satrans_cross_desc {
    int32_t B, N, L;
    int32_t matrix;                         /* 0: vector form, 1: matrix form */
    const float* x0;                        /* [B, N] */
    const float* kernels;                   /* [L, N] or [L, N, N] */
    const float* bias;                      /* [L, N] */
} satrans_cross_desc;
typedef struct satrans_cross_grads {
    float* kernels;
    float* bias;
} satrans_cross_grads;
int64_t satrans_cross_saved_floats(const satrans_cross_desc* d);
int64_t satrans_cross_workspace_floats(const satrans_cross_desc* d);
int satrans_cross_fwd(const satrans_cross_desc* d, float* result, float* saved, void* stream);
int satrans_cross_bwd(const satrans_cross_desc* d, const float* dresult, float* dx, const float* saved, float* workspace,
                      const satrans_cross_grads* g, void* stream);

/* FiBiNET (deepctr-torch's SENETLayer and BilinearInteraction, which the reference's models/fibinet.py:51-52,93-95 calls, and
 * the half of its forward behind the lookup).  With e [B, F, D], R = max(1, F / reduction_ratio), pairs (i, j), i < j, in
 * itertools.combinations order, P = F (F - 1) / 2, pair p = i (2 F - i - 1) / 2 + j - i - 1:
 *     SENet      z[b,f] = mean_d e[b,f,:]    hid = relu(z w1^T)    a = relu(hid w2^T)    v = e * a[:,:,None]
 *                w1 [R, F], w2 [F, R] (the excitation's two bias-free Linears)
 *     bilinear   r_p = (W_w(p) e_i) * e_j    W [nW, D, D] (Linear weights, [d_out, d_in]);  w(p) = 0 (ALL, nW = 1), i (EACH,
 *                nW = F; the last is never used and its gradient comes out zero), p (INTERACTION, nW = P)
 *                with a [B, F]:  s_p = a_i a_j r_p, which is the product over v = e * a (one D x D product serves both)
 *     head       x = [ s_0 .. s_{P-1} | r_0 .. r_{P-1} | dense ]  [B, 2 P D + dense_dim];  hidden layers relu(x W^T + b);
 *                logit [B, 1] = h dnn_linear_w^T + out_bias
 * fp32 throughout.  2 to SATRANS_FIBINET_MAX_FIELDS fields, D up to SATRANS_FIBINET_MAX_DIM (any D, not only multiples of 4),
 * up to SATRANS_MMOE_MAX_HIDDEN hidden layers (none: dnn_linear sits on x), any positive B whose launches fit 2^31 workgroups
 * (SATRANS_E_UNSUPPORTED beyond); all of that is decided before a device is touched.
 * satrans_senet_fwd: saved = a [B, F], then hid [B, R]; v [B, F, D] is written when not null.  satrans_senet_bwd takes da
 * [B, F] and / or dv [B, F, D] (either may be null, not both), ADDS the input gradient into de [B, F, D] and writes g->w1,
 * g->w2; workspace = 2 ceil(B / SATRANS_FIBINET_SENET_ROW_CHUNK) F R floats.
 * satrans_bilinear_fwd: out [B, P D] = r, or with d->a: out [B, 2 P D] = [ s | r ].  satrans_bilinear_bwd takes dout and out in
 * that layout, WRITES de [B, F, D], da [B, F] (with d->a) and dw [nW, D, D]; workspace =
 * ceil(B / SATRANS_FIBINET_DW_ROW_CHUNK) nW D D floats.
 * satrans_fibinet_fwd: saved = a, hid, x [B, 2 P D + dense_dim], the hidden rows.  satrans_fibinet_bwd WRITES demb [B, F, D],
 * ddense [B, dense_dim] (null when dense_dim = 0) and every gradient of g.
 * No floating-point atomics: equal inputs give equal bits, and a sample's logit and demb row are the same bits alone as
 * inside a batch. */
#define SATRANS_FIBINET_MAX_FIELDS 64
#define SATRANS_FIBINET_MAX_DIM 128
#define SATRANS_FIBINET_DW_ROW_CHUNK 256
#define SATRANS_FIBINET_SENET_ROW_CHUNK 32
#define SATRANS_BILINEAR_ALL 0
#define SATRANS_BILINEAR_EACH 1
#define SATRANS_BILINEAR_INTERACTION 2
typedef struct satrans_senet_desc {
    int32_t B, F, D, R;
    const float* e;                         /* [B, F, D] */
    const float* w1;                        /* [R, F] */
    const float* w2;                        /* [F, R] */
} satrans_senet_desc;
typedef struct satrans_senet_grads {
    float* w1;
    float* w2;
} satrans_senet_grads;
int64_t satrans_senet_saved_floats(const satrans_senet_desc* d);
int64_t satrans_senet_workspace_floats(const satrans_senet_desc* d);
int satrans_senet_fwd(const satrans_senet_desc* d, float* v, float* saved, void* stream);
int satrans_senet_bwd(const satrans_senet_desc* d, const float* da, const float* dv, const float* saved, float* de, float* workspace,
                      const satrans_senet_grads* g, void* stream);
typedef struct satrans_bilinear_desc {
    int32_t B, F, D;
    int32_t type;                           /* SATRANS_BILINEAR_* */
    const float* e;                         /* [B, F, D] */
    const float* w;                         /* [nW, D, D] */
    const float* a;                         /* [B, F], or null: the raw block only */
} satrans_bilinear_desc;
int64_t satrans_bilinear_workspace_floats(const satrans_bilinear_desc* d);
int satrans_bilinear_fwd(const satrans_bilinear_desc* d, float* out, void* stream);
int satrans_bilinear_bwd(const satrans_bilinear_desc* d, const float* dout, const float* out, float* de, float* da, float* workspace,
                         float* dw, void* stream);
typedef struct satrans_fibinet_desc {
    int32_t B, F, D;
    int32_t type;                           /* SATRANS_BILINEAR_* */
    int32_t R, dense_dim, n_dnn, reserved;
    int32_t width[SATRANS_MMOE_MAX_HIDDEN];
    int32_t reserved2;
    const float* emb;                       /* [B, F, D] */
    const float* dense;                     /* [B, dense_dim], null when dense_dim = 0 */
    const float* se_w1;
    const float* se_w2;
    const float* bilinear_w;
    const float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_linear_w;              /* [1, last width] */
    const float* out_bias;                  /* [1] */
} satrans_fibinet_desc;
typedef struct satrans_fibinet_grads {
    float* se_w1;
    float* se_w2;
    float* bilinear_w;
    float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_linear_w;
    float* out_bias;
} satrans_fibinet_grads;
int64_t satrans_fibinet_saved_floats(const satrans_fibinet_desc* d);
int64_t satrans_fibinet_workspace_floats(const satrans_fibinet_desc* d);
int satrans_fibinet_fwd(const satrans_fibinet_desc* d, float* logit, float* saved, void* stream);
int satrans_fibinet_bwd(const satrans_fibinet_desc* d, const float* dlogit, float* demb, float* ddense, const float* saved,
                        float* workspace, const satrans_fibinet_grads* g, void* stream);

/* PNN (deepctr-torch's InnerProductLayer and OutterProductLayer, which the reference's models/pnn.py:14,61,65 calls, and
 * pnn.py:91-114).  With e [B, F, D], pairs (i, j), i < j, in itertools.combinations order, P = F (F - 1) / 2, pair
 * p = i (2 F - i - 1) / 2 + j - i - 1:
 *     inner        ip[b,p] = sum_d e_i[d] e_j[d]
 *     outer MAT    op[b,p] = sum_n ( sum_k e_i[k] kernel[n,p,k] ) e_j[n]          kernel [D, P, D]
 *     outer VEC    op[b,p] = sum_d e_i[d] e_j[d] kernel[p,d]                      kernel [P, D]
 *     outer NUM    op[b,p] = kernel[p,0] * sum_d e_i[d] e_j[d]                    kernel [P, 1]
 *     head         x = [ flatten(e) (F D) | ip (P, if use_inner) | op (P, if use_outer) | dense ];  hidden layers
 *                  relu(x W^T + b);  logit [B, 1] = h dnn_linear_w^T + out_bias
 * Backward, with g_p[b] the upstream gradient of one product column:
 *     inner / NUM / VEC   de_i += g_p c_p * e_j,  de_j += g_p c_p * e_i;  c_p = 1 (inner), kernel[p] (NUM), kernel[p,:] (VEC);
 *                         dkernel[p] = sum_b g_p <e_i, e_j> (NUM);  dkernel[p,d] = sum_b g_p e_i[d] e_j[d] (VEC)
 *     MAT                 de_j += K_p (g_p e_i),  de_i += K_p^T (g_p e_j),  dkernel[n,p,k] = sum_b g_p e_j[n] e_i[k]
 *                         (K_p = kernel[:, p, :], read in place: row n at kernel + (n P + p) D)
 * fp32 throughout.  2 to SATRANS_PNN_MAX_FIELDS fields, D up to SATRANS_PNN_MAX_DIM (any D, not only multiples of 4), up to
 * SATRANS_MMOE_MAX_HIDDEN hidden layers (none: dnn_linear sits on x), any positive B whose launches fit 2^31 workgroups
 * (SATRANS_E_UNSUPPORTED beyond); all of that is decided before a device is touched.
 * satrans_inner_product_fwd: out [B, P].  satrans_inner_product_bwd takes dout [B, P] and WRITES de [B, F, D].
 * satrans_outer_product_fwd: out [B, P].  satrans_outer_product_bwd takes dout [B, P] and WRITES de [B, F, D] and dkernel (the
 * kernel's shape); workspace = ceil(B / SATRANS_PNN_DW_ROW_CHUNK) P D floats times D (MAT) or 1 (VEC, NUM).
 * satrans_pnn_fwd: saved = x [B, F D + P use_inner + P use_outer + dense_dim], the hidden rows.  satrans_pnn_bwd WRITES demb
 * [B, F, D], ddense [B, dense_dim] (null when dense_dim = 0) and every gradient of g (g->kernel and d->kernel may be null
 * without use_outer).  With neither product the head is the DNN over [ flatten(e) | dense ].
 * No floating-point atomics: equal inputs give equal bits, and a sample's logit and demb row are the same bits alone as
 * inside a batch. */
#define SATRANS_PNN_MAX_FIELDS 64
#define SATRANS_PNN_MAX_DIM 128
#define SATRANS_PNN_DW_ROW_CHUNK 256
#define SATRANS_PNN_KERNEL_MAT 0
#define SATRANS_PNN_KERNEL_VEC 1
#define SATRANS_PNN_KERNEL_NUM 2
typedef struct satrans_inner_product_desc {
    int32_t B, F, D, reserved;
    const float* e;                         /* [B, F, D] */
} satrans_inner_product_desc;
int satrans_inner_product_fwd(const satrans_inner_product_desc* d, float* out, void* stream);
int satrans_inner_product_bwd(const satrans_inner_product_desc* d, const float* dout, float* de, void* stream);
typedef struct satrans_outer_product_desc {
    int32_t B, F, D;
    int32_t kernel_type;                    /* SATRANS_PNN_KERNEL_* */
    const float* e;                         /* [B, F, D] */
    const float* kernel;                    /* [D, P, D] (MAT), [P, D] (VEC), [P, 1] (NUM) */
} satrans_outer_product_desc;
int64_t satrans_outer_product_workspace_floats(const satrans_outer_product_desc* d);
int satrans_outer_product_fwd(const satrans_outer_product_desc* d, float* out, void* stream);
int satrans_outer_product_bwd(const satrans_outer_product_desc* d, const float* dout, float* de, float* workspace, float* dkernel,
                              void* stream);
typedef struct satrans_pnn_desc {
    int32_t B, F, D;
    int32_t use_inner, use_outer;
    int32_t kernel_type;                    /* SATRANS_PNN_KERNEL_* (read with use_outer) */
    int32_t dense_dim, n_dnn;
    int32_t width[SATRANS_MMOE_MAX_HIDDEN];
    int32_t reserved;
    const float* emb;                       /* [B, F, D] */
    const float* dense;                     /* [B, dense_dim], null when dense_dim = 0 */
    const float* kernel;                    /* the outer product's, null without use_outer */
    const float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_linear_w;              /* [1, last width] */
    const float* out_bias;                  /* [1] */
} satrans_pnn_desc;
typedef struct satrans_pnn_grads {
    float* kernel;
    float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_linear_w;
    float* out_bias;
} satrans_pnn_grads;
int64_t satrans_pnn_saved_floats(const satrans_pnn_desc* d);
int64_t satrans_pnn_workspace_floats(const satrans_pnn_desc* d);
int satrans_pnn_fwd(const satrans_pnn_desc* d, float* logit, float* saved, void* stream);
int satrans_pnn_bwd(const satrans_pnn_desc* d, const float* dlogit, float* demb, float* ddense, const float* saved, float* workspace,
                    const satrans_pnn_grads* g, void* stream);

/* FM, BiInteractionPooling and AFMLayer of deepctr-torch 0.2.9, which the reference's models/deepfm.py, nfm.py and afm.py
 * import, and the halves of their forward behind the lookup (deepfm.py:87-113, nfm.py:73-83, afm.py:66-73).  With e [B, F, D]
 * and S = sum_f e_f:
 *     FM        out[b]   = 0.5 sum_d (S_d^2 - sum_f e_fd^2)                       de_f  = dout (S - e_f)
 *     bipool    out[b,d] = 0.5 (S_d^2 - sum_f e_fd^2)                             de_fd = dout_d (S_d - e_fd)
 *     AFM       over the pairs p = (i, j), i < j, in itertools.combinations order (P = F (F - 1) / 2):  x_p = e_i * e_j,
 *               t_p = relu(x_p attention_W + attention_b), a = softmax_p(t_p projection_h), ao = sum_p a_p x_p,
 *               out[b] = ao . projection_p (+ linear_logit[b] + out_bias[0], each when not null)
 *     DEEPFM    logit = linear_logit + FM(e) (use_fm) + dnn_linear(dnn([ flatten(e) | dense ])) (n_dnn > 0) + out_bias
 *     NFM       logit = linear_logit + dnn_linear(dnn([ bipool(e) | dense ])) + out_bias          (n_dnn > 0 required)
 * fp32 throughout.  2 to SATRANS_FM_MAX_FIELDS fields, D up to SATRANS_FM_MAX_DIM (any D), A from 1 to SATRANS_AFM_MAX_FACTOR,
 * up to SATRANS_MMOE_MAX_HIDDEN hidden layers, any positive B whose launches fit the grid; SATRANS_E_UNSUPPORTED beyond, decided
 * before a device is touched.
 * satrans_fm_fwd: out [B].  satrans_bipool_fwd: out [B, D].  Their _bwd take dout of that shape and WRITE de [B, F, D].
 * satrans_afm_fwd: out [B]; saved = a [B, P] (deepctr's normalized_att_score), ao [B, D]: B (P + D) floats.  satrans_afm_bwd
 * takes dout [B] and WRITES de and every gradient of g (g->out_bias, the sum of dout, may be null when d->out_bias is); its
 * workspace is one partial of D A + 2 A + D floats per workgroup, at most SATRANS_AFM_MAX_WORKGROUPS of them, merged in
 * workgroup order.  The gradient of linear_logit is dout itself.
 * satrans_fmhead_fwd: logit [B, 1]; saved = the DNN input [B, (DEEPFM: F D, NFM: D) + dense_dim], the hidden rows (nothing
 * without a DNN).  satrans_fmhead_bwd WRITES demb [B, F, D], ddense [B, dense_dim] (null when dense_dim = 0 or without a DNN)
 * and every gradient of g; the gradient of linear_logit is dlogit itself.
 * No floating-point atomics: equal inputs give equal bits, and a sample's out / logit and de row are the same bits alone as
 * inside a batch. */
#define SATRANS_FM_MAX_FIELDS 64
#define SATRANS_FM_MAX_DIM 128
#define SATRANS_AFM_MAX_FACTOR 64
#define SATRANS_AFM_MAX_WORKGROUPS 1024
#define SATRANS_FMHEAD_DEEPFM 0
#define SATRANS_FMHEAD_NFM 1
typedef struct satrans_fm_desc {
    int32_t B, F, D, reserved;
    const float* e;                         /* [B, F, D] */
} satrans_fm_desc;
int satrans_fm_fwd(const satrans_fm_desc* d, float* out, void* stream);
int satrans_fm_bwd(const satrans_fm_desc* d, const float* dout, float* de, void* stream);
int satrans_bipool_fwd(const satrans_fm_desc* d, float* out, void* stream);
int satrans_bipool_bwd(const satrans_fm_desc* d, const float* dout, float* de, void* stream);
typedef struct satrans_afm_desc {
    int32_t B, F, D, A;
    const float* e;                         /* [B, F, D] */
    const float* attention_W;               /* [D, A] */
    const float* attention_b;               /* [A] */
    const float* projection_h;              /* [A, 1] */
    const float* projection_p;              /* [D, 1] */
    const float* linear_logit;              /* [B, 1], null: none */
    const float* out_bias;                  /* [1], null: none */
} satrans_afm_desc;
typedef struct satrans_afm_grads {
    float* attention_W;
    float* attention_b;
    float* projection_h;
    float* projection_p;
    float* out_bias;
} satrans_afm_grads;
int64_t satrans_afm_saved_floats(const satrans_afm_desc* d);
int64_t satrans_afm_workspace_floats(const satrans_afm_desc* d);
int satrans_afm_fwd(const satrans_afm_desc* d, float* out, float* saved, void* stream);
int satrans_afm_bwd(const satrans_afm_desc* d, const float* dout, float* de, const float* saved, float* workspace,
                    const satrans_afm_grads* g, void* stream);
typedef struct satrans_fmhead_desc {
    int32_t B, F, D;
    int32_t kind;                           /* SATRANS_FMHEAD_* */
    int32_t use_fm;                         /* DEEPFM: the FM term */
    int32_t dense_dim, n_dnn;
    int32_t reserved;
    int32_t width[SATRANS_MMOE_MAX_HIDDEN];
    int32_t reserved2;
    const float* emb;                       /* [B, F, D] */
    const float* dense;                     /* [B, dense_dim], null when dense_dim = 0 */
    const float* linear_logit;              /* [B, 1], null: none */
    const float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_linear_w;              /* [1, last width] */
    const float* out_bias;                  /* [1] */
} satrans_fmhead_desc;
typedef struct satrans_fmhead_grads {
    float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_linear_w;
    float* out_bias;
} satrans_fmhead_grads;
int64_t satrans_fmhead_saved_floats(const satrans_fmhead_desc* d);
int64_t satrans_fmhead_workspace_floats(const satrans_fmhead_desc* d);
int satrans_fmhead_fwd(const satrans_fmhead_desc* d, float* logit, float* saved, void* stream);
int satrans_fmhead_bwd(const satrans_fmhead_desc* d, const float* dlogit, float* demb, float* ddense, const float* saved,
                       float* workspace, const satrans_fmhead_grads* g, void* stream);

/* InteractingLayer of deepctr-torch 0.2.9, which the reference's models/autoint.py builds (autoint.py:13,75-76), and the half of
 * AutoInt.forward behind the lookup (autoint.py:93-121).  It is NOT satrans_selfatt_*: no W_Out, no dropout, no LayerNorm.
 * x [B, F, D], H heads of dh = D / H columns, weights [D, D] applied as x W:
 *     q, k, v, r = x W_Query, x W_key, x W_Value, x W_Res;   p = softmax_j(q_i . k_j (/ sqrt(dh) unless SATRANS_NO_SCALING)) per
 *     (sample, head);   y = relu(p v + r)   (no r with SATRANS_NO_RES, and then w_res is not read)
 *     AUTOINT   logit = [ flatten(layer_L(... layer_1(emb))) | dnn([ flatten(emb) | dense ]) ] dnn_linear_w^T + out_bias
 *               (without a DNN, n_dnn = 0: the first block alone, and dense is not read)
 * fp32 throughout.  D in {16, 32, 64}, dh in {8, 16, 32}, 2 <= F <= 64, any B >= 1; the size functions return -1 for anything else
 * and the launches SATRANS_E_UNSUPPORTED, decided before a device is touched.
 * satrans_interacting_fwd: one launch.  y [B, F, D]; att (or null) [H, B, F, F], deepctr's normalized_att_scores; saved = the
 * softmax rows' (max, sum): 2 B H F floats, all written.  satrans_interacting_bwd takes y (for the relu mask) and dy, recomputes q, k, v from
 * d->x, WRITES dx [B, F, D] and g_w = the gradients of W_Query, W_key, W_Value (, W_Res) as one [3 or 4, D, D] block; scratch is
 * one such block per workgroup, at most SATRANS_INTERACTING_MAX_WORKGROUPS of them, merged in workgroup order.
 * satrans_autoint_fwd: logit [B, 1]; att (or null): n_layers pointers, each null or [H, B, F, F]; saved = the layers' outputs
 * [n_layers, B, F, D], their statistics, and with a DNN its input [B, F D + dense_dim] and hidden rows.  satrans_autoint_bwd
 * WRITES demb [B, F, D], ddense [B, dense_dim] (null when dense_dim = 0 or without a DNN) and every gradient of g; g->int_w[l]
 * is layer l's [3 or 4, D, D] block.
 * No floating-point atomics: equal inputs give equal bits, and a sample's y / logit are the same bits alone as inside a batch. */
#define SATRANS_INTERACTING_MAX_WORKGROUPS 512
#define SATRANS_AUTOINT_MAX_LAYERS 8
typedef struct satrans_interacting_desc {
    int32_t B, F, D, H;
    uint32_t flags;                         /* SATRANS_NO_RES, SATRANS_NO_SCALING */
    int32_t reserved;
    const float* x;                         /* [B, F, D] */
    const float* w_query;                   /* [D, D] */
    const float* w_key;
    const float* w_value;
    const float* w_res;                     /* null with SATRANS_NO_RES */
} satrans_interacting_desc;
int64_t satrans_interacting_saved_floats(const satrans_interacting_desc* d);
int64_t satrans_interacting_scratch_floats(const satrans_interacting_desc* d);
int satrans_interacting_fwd(const satrans_interacting_desc* d, float* y, float* att, float* saved, void* stream);
int satrans_interacting_bwd(const satrans_interacting_desc* d, const float* y, const float* dy, float* dx, const float* saved,
                            float* scratch, float* g_w, void* stream);
typedef struct satrans_autoint_desc {
    int32_t B, F, D, H;
    uint32_t flags;                         /* SATRANS_NO_RES, SATRANS_NO_SCALING */
    int32_t n_layers, dense_dim, n_dnn;
    int32_t width[SATRANS_MMOE_MAX_HIDDEN];
    int32_t reserved;
    const float* emb;                       /* [B, F, D] */
    const float* dense;                     /* [B, dense_dim], null when dense_dim = 0 */
    const float* w_query[SATRANS_AUTOINT_MAX_LAYERS];
    const float* w_key[SATRANS_AUTOINT_MAX_LAYERS];
    const float* w_value[SATRANS_AUTOINT_MAX_LAYERS];
    const float* w_res[SATRANS_AUTOINT_MAX_LAYERS];
    const float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_linear_w;              /* [1, F D + last width] (n_dnn = 0: [1, F D]) */
    const float* out_bias;                  /* [1] */
} satrans_autoint_desc;
typedef struct satrans_autoint_grads {
    float* int_w[SATRANS_AUTOINT_MAX_LAYERS];
    float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_linear_w;
    float* out_bias;
} satrans_autoint_grads;
int64_t satrans_autoint_saved_floats(const satrans_autoint_desc* d);
int64_t satrans_autoint_workspace_floats(const satrans_autoint_desc* d);
int satrans_autoint_fwd(const satrans_autoint_desc* d, float* logit, float* const* att, float* saved, void* stream);
int satrans_autoint_bwd(const satrans_autoint_desc* d, const float* dlogit, float* demb, float* ddense, const float* saved,
                        float* workspace, const satrans_autoint_grads* g, void* stream);

/* ESMM's two towers (models/esmm.py:84-96) and WDL's DNN-only head (models/wdl.py:75-79), with dropout inside the DNNs.  Also
 * additive in ABI version 7: new structs and new symbols only.  Nothing is routed: `towers` DNNs of equal widths over all rows,
 *     h_{t,l} = drop(relu(h_{t,l-1} dnn_w[l][t]^T + dnn_b[l][t])),  h_{t,0} = x,  l = 1 .. n_dnn;   logit_t = h_{t,n_dnn} final_w[t]^T
 *     towers = 2 (ESMM)   p_t = sigmoid(logit_t + out_bias[0]);  out [B, 2] = (p_0, p_0 p_1)        (ctr, ctcvr: probabilities)
 *     towers = 1 (WDL)    out [B, 1] = logit_0 + out_bias[0]                                         (a logit)
 * x [B, C]; dnn_w[l] [towers, n_l, n_{l-1}] (n_0 = C), dnn_b[l] [towers, n_l], final_w [towers, n_last] (no final bias, as in
 * the reference), out_bias [1].  fp32 throughout, products on the exact f32-input MFMA.  1 to SATRANS_MMOE_MAX_HIDDEN hidden
 * layers; C and the widths are any positive integers.  Row tiles and weight-gradient chunks are those of the MMoE head.
 * Layer 1 of both towers is one product of N = towers * n_1, later layers are block-diagonal.  Two forms of the tail, chosen by
 * satrans_esmm_set_forward (process-wide; returns the previous mode, or SATRANS_E_BADARG), with the same bits in out and saved,
 * with and without dropout:
 *     1, the default   composed: the last hidden layer and the final layer are two launches of the tile product (the second
 *                      with N = 1), then for towers = 2 a pointwise kernel
 *     0                fused: the last hidden layer, the final layer, the sigmoids and the product are ONE launch (with
 *                      n_dnn = 1 the whole head): per row the chain logit_t = fmaf(h[n], final_w[t][n], logit_t), n ascending
 * The fused tail was measured against the composed form and was not faster (profiles/esmm_time.txt), so it is not the default.
 * Dropout: with SATRANS_TRAIN in flags and drop_p > 0, element (row, n) of tower t's hidden layer l (0-based) is kept iff
 *     drop_keep(drop_sample_key(drop_site_key(seed, step, l, t), row + row_offset), n, drop_threshold(drop_p))       (csrc/rng.h)
 * and a kept element is scaled by 1.0f / (1.0f - drop_p); oracle.satrans_oracle.dropout_keep(seed, step, l, t, row + row_offset,
 * n, p) restates it.  Without SATRANS_TRAIN, or with drop_p = 0, the kernels without the option are launched.  The backward
 * must see the forward's seed, step, row_offset, flags and drop_p (it reads only the scale: no mask is regenerated - a saved
 * h > 0 is "kept and past the relu").
 * saved: the hidden rows, layer by layer [B, towers * n_l] (tower t in columns [t n_l, (t + 1) n_l)), dropped-out and scaled in
 * training; then, with towers = 2, (p_0, p_1) [B, 2].  The forward needs no workspace; the backward's holds two
 * [B, widest stacked row] dz buffers and the per-chunk partials of the layer in hand.  From dout [B, towers]:
 *     dp_0 = dout_0 + dout_1 p_1,  dp_1 = dout_1 p_0,  dlogit_t = dp_t p_t (1 - p_t)          (towers = 1: dlogit_0 = dout)
 *     dz_t[row, n] = h_t[row, n] > 0 ? dlogit_t final_w[t][n] (* scale) : 0;   d out_bias = sum over rows of (dlogit_0 + dlogit_1)
 * The backward WRITES dx [B, C] and every gradient of satrans_esmm_grads, each of the shape of its parameter.  No
 * floating-point atomics: chunks merge in chunk order, so equal inputs give equal bits, and a sample alone gives the bits it
 * gives inside a batch (its out row and dx row; with dropout when row_offset places it where it sat).  Every size and grid is
 * decided before a device is touched: SATRANS_E_UNSUPPORTED beyond 2^31 workgroups. */
typedef struct satrans_esmm_desc {
    int32_t B, C;
    int32_t towers;                         /* 1 = WDL, 2 = ESMM */
    int32_t n_dnn;                          /* hidden layers of a tower */
    int32_t width[SATRANS_MMOE_MAX_HIDDEN];
    uint32_t flags;                         /* SATRANS_TRAIN */
    float drop_p;                           /* 0 <= p < 1 */
    uint32_t seed, step;
    uint32_t row_offset;                    /* of row 0 in the global batch, for the masks */
    const float* x;                         /* [B, C] */
    const float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    const float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    const float* final_w;
    const float* out_bias;
} satrans_esmm_desc;
typedef struct satrans_esmm_grads {
    float* dnn_w[SATRANS_MMOE_MAX_HIDDEN];
    float* dnn_b[SATRANS_MMOE_MAX_HIDDEN];
    float* final_w;
    float* out_bias;
} satrans_esmm_grads;
int64_t satrans_esmm_saved_floats(const satrans_esmm_desc* d);
int64_t satrans_esmm_workspace_floats(const satrans_esmm_desc* d);
int satrans_esmm_fwd(const satrans_esmm_desc* d, float* out, float* saved, void* stream);
int satrans_esmm_bwd(const satrans_esmm_desc* d, const float* dout, float* dx, const float* saved, float* workspace,
                     const satrans_esmm_grads* g, void* stream);
int satrans_esmm_set_forward(int composed);

/* Backward of one layer.  Recomputes the forward from d->x (same dropout counters), so nothing but
 * the layer input is kept between the passes.
 *   dy        [B,F,D] gradient of the layer output
 *   dx        [B,F,D] gradient of the layer input (written)
 *   slabs     workspace, satrans_layer_bwd_slab_floats(d) floats; per-workgroup partial weight gradients
 *   g_*       gradients of the parameters, ACCUMULATED (+=) in a fixed order (bitwise reproducible):
 *             g_wq,g_wk,g_wv,g_wo [D,D]; g_ln [2,D]; g_lnq [2,D]; g_lnk [2,D] (gamma row then beta row);
 *             g_tab_q, g_tab_k [S, tab_stride] (may alias when tab_q == tab_k).                        */
int64_t satrans_layer_bwd_slab_floats(const satrans_layer_desc* d);
int satrans_layer_bwd(const satrans_layer_desc* d, const float* dy, float* dx, float* slabs,
                      float* g_wq, float* g_wk, float* g_wv, float* g_wo, float* g_ln, float* g_lnq,
                      float* g_lnk, float* g_tab_q, float* g_tab_k, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Head: flatten + [dense columns] + Linear(->1) + sigmoid (reference satrans.py:244-255) and, for
 * training, BCE(reduction='sum') (meta_basemodel.py:317) with its backward in the same launch.
 *   a        [B, F*D] last layer output
 *   dense    float matrix holding the DenseFeat columns (X itself when ids travel as floats), row stride
 *            dense_stride, dense_cols [n_dense] int32 (device) = its columns in feature order; may be null
 *   w        [F*D + n_dense], bias [1]
 *   prob     [B] sigmoid(logit);  logit optional [B]
 *   y        optional labels [B] (fp32).  When given:
 *              loss_sum[0] (double) += BCE sum over the batch (per-block partials added in block order),
 *              da [B,F*D] = dlogit * w[:F*D],  g_w += sum_b dlogit_b * [a_b | dense_b],  g_b += sum dlogit,
 *              scratch: satrans_head_scratch_floats(B, FD, n_dense) floats
 * ---------------------------------------------------------------------------------------------- */
int satrans_head(const float* a, const float* dense, int64_t dense_stride, const int32_t* dense_cols, int n_dense,
                 int B, int FD, const float* w, const float* bias, float* prob, float* logit, const float* y,
                 double* loss_sum, float* da, float* g_w, float* g_b, float* scratch, void* stream);

/* The same with the loss of `compile(loss=...)` (models/meta_basemodel.py:642-653, all reduction='sum' in fit):
 * SATRANS_LOSS_BCE binary_cross_entropy, SATRANS_LOSS_MSE F.mse_loss, SATRANS_LOSS_MAE F.l1_loss on the probability. */
#define SATRANS_LOSS_BCE 0
#define SATRANS_LOSS_MSE 1
#define SATRANS_LOSS_MAE 2
int satrans_head_loss(const float* a, const float* dense, int64_t dense_stride, const int32_t* dense_cols, int n_dense, int B,
                      int FD, const float* w, const float* bias, float* prob, float* logit, const float* y, double* loss_sum,
                      float* da, float* g_w, float* g_b, float* scratch, int loss_kind, void* stream);

/* Prediction, loss (reduction='sum') and the loss's gradient for a column of logits, for the models whose head ends in a logit
 * (reference models/basemodel.py:299-315: `model(x).squeeze()`, `loss_func(y_pred, y, reduction='sum')`, and their backward;
 * PredictionLayer: sigmoid for task='binary', the identity for task='regression').  The arithmetic per sample is
 * satrans_head_loss's: at the same logit `pred` and `dz` carry the bits of its `prob` and `dlogit`.
 *   z        logit of sample b at z[b * z_stride] (z_stride in elements: a column of a [B, T] block)
 *   y        [B] labels, or NULL: prediction only (`dz`, `loss_sum`, `partial` are not touched)
 *   pred     [B]
 *   dz       [B] d(loss sum)/dz, or NULL (evaluation)
 *   loss_sum [1] double, += the sum of the per-sample fp32 losses, each widened to double and added in a fixed order
 *            (lane, wave, block, then the blocks in index order): two runs give the same bits; no floating-point atomics
 *   partial  satrans_point_loss_partials(B) doubles of scratch (may be NULL when B <= 256)
 * At most two launches.  SATRANS_PRED_LINEAR with SATRANS_LOSS_BCE takes z itself as the probability, as the reference
 * would. */
#define SATRANS_PRED_SIGMOID 0
#define SATRANS_PRED_LINEAR 1
int64_t satrans_point_loss_partials(int B);
int satrans_point_loss(const float* z, int64_t z_stride, const float* y, int B, int pred_kind, int loss_kind, float* pred, float* dz,
                       double* loss_sum, double* partial, void* stream);

/* The routed form, for a [B, T] block of per-task predictions where a row's loss is taken on the column of its own task
 * (reference models/mtl_basemodel.py:268-269, the masked per-task loss sum; :376-378, predict's assembly).  Additive in ABI
 * version 7: a new symbol only.
 *   z        [B, T], row b at z + b * z_stride (z_stride >= T, in elements)
 *   task     [B] int32: the column of row b (scenario id minus domain_id_offset)
 *   T        a runtime value, any T >= 1
 *   dz       [B, T] contiguous, or NULL; EVERY entry is written (no zero-fill by the caller): dz[b, task[b]] = the gradient,
 *            0 elsewhere
 * A row with 0 <= task[b] < T computes satrans_point_loss's expressions on z[b, task[b]]: the same bits.  Any other row belongs
 * to no task's mask, as in the reference: pred[b] = 0, nothing added to the sum, a zero dz row.  y, pred, loss_sum, partial
 * (satrans_point_loss_partials(B)), the order of the sum and the launch count are satrans_point_loss's. */
int satrans_point_loss_routed(const float* z, int64_t z_stride, const int32_t* task, const float* y, int B, int T, int pred_kind,
                              int loss_kind, float* pred, float* dz, double* loss_sum, double* partial, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The LAST layer of a training step with the head fused in: one launch (plus two small fixed-order reductions) that replaces
 *   satrans_layer_fwd(last layer) + satrans_head_loss + satrans_layer_bwd(last layer)
 * i.e. reference satrans.py:50-100 (recomputed from the layer input, as satrans_layer_bwd does anyway), :244-255 (flatten +
 * dense columns + Linear + sigmoid), meta_basemodel.py:317 (loss, reduction='sum') and their backward.  A workgroup tile holds
 * whole samples, so the logit of a sample is a sum over rows the tile has in registers: neither the layer output [B,F,D] nor its
 * gradient is written or read, and the step runs L - 1 forward launches instead of L.
 *   d          the last layer (d->x = its input, flags / dropout counters as for its forward)
 *   h          head operands: w [F*D + n_dense], bias [1], labels [B] (fp32); dense / dense_stride / h_dense_cols as in
 *              satrans_head, except that h_dense_cols is a HOST array (the kernel takes the columns by value; n_dense <= 2);
 *              outputs prob [B], logit [B] (optional), loss_sum[0] (double) += the batch's loss sum, g_w / g_b ACCUMULATED;
 *              scratch: satrans_layer_bwd_head_scratch_floats(d, n_dense) floats
 *   dx, slabs, g_* as satrans_layer_bwd.
 * Built for the fused MetaNet shapes (D,U,H) = (32,64,4), (16,32,2) with fp32 products; satrans_layer_bwd_head_supported says
 * whether a layer / head pair can take this path (callers fall back to the three separate calls otherwise). */
typedef struct satrans_head_desc {
    const float* w;
    const float* bias;
    const float* labels;
    const float* dense;
    int64_t dense_stride;
    const int32_t* h_dense_cols; /* HOST array [n_dense] */
    int32_t n_dense, loss_kind;  /* SATRANS_LOSS_* */
    float* prob;
    float* logit;
    double* loss_sum;
    float* g_w;
    float* g_b;
    float* scratch;
} satrans_head_desc;
int satrans_layer_bwd_head_supported(const satrans_layer_desc* d, const satrans_head_desc* h);
/* satrans_stack_fwd_bf16 with the head behind it in the same launch (evaluation: satrans.py:236-255): h->w, h->bias, the dense
 * columns as above, outputs h->prob [B] and h->logit [B] (optional); labels / loss / gradients of `h` are not used.  A tile holds
 * whole samples, so the last layer's rows never leave LDS; head_kernel's summation order, i.e. the bits of satrans_head. */
int satrans_stack_fwd_bf16_head(int n, const satrans_layer_desc* const* descs, const satrans_head_desc* h, void* stream);
int64_t satrans_layer_bwd_head_scratch_floats(const satrans_layer_desc* d, int n_dense);
int satrans_layer_bwd_head(const satrans_layer_desc* d, const satrans_head_desc* h, float* dx, float* slabs, float* g_wq,
                           float* g_wk, float* g_wv, float* g_wo, float* g_ln, float* g_lnq, float* g_lnk, float* g_tab_q,
                           float* g_tab_k, void* stream);

/* The same two calls without their reduction launches, and ONE reduction launch for all layers of a step.  satrans_layer_bwd ends
 * with a fixed-order reduction of per-workgroup slabs (~10 us of a mostly idle GPU per layer); a training step can instead launch
 * its L backward kernels back to back - a slab buffer of satrans_layer_bwd_slab_floats(d) floats PER LAYER - and reduce them all,
 * together with the fused head's partial rows, in one launch on whichever stream suits it (the engine runs it on a side stream
 * underneath the touched-row optimizer kernels).  Same arithmetic and order per layer: the same bits as the per-layer calls.
 *   h_descs / h_slabs / h_grads   HOST arrays of n entries (n <= 8); the layers must share batch, bucketing, shape and flags
 *   head                          the descriptor given to satrans_layer_bwd_head_launch, or NULL
 * Fused kernels only: satrans_layer_bwd_deferred_supported says whether a layer can take this route. */
typedef struct satrans_layer_grads {
    float *g_wq, *g_wk, *g_wv, *g_wo, *g_ln, *g_lnq, *g_lnk, *g_tab_q, *g_tab_k;
} satrans_layer_grads;
int satrans_layer_bwd_deferred_supported(const satrans_layer_desc* d);
int satrans_layer_bwd_launch(const satrans_layer_desc* d, const float* dy, float* dx, float* slabs, void* stream);
int satrans_layer_bwd_head_launch(const satrans_layer_desc* d, const satrans_head_desc* h, float* dx, float* slabs, void* stream);
int satrans_layer_bwd_reduce(int n, const satrans_layer_desc* const* h_descs, float* const* h_slabs,
                             const satrans_layer_grads* h_grads, const satrans_head_desc* head, void* stream);

/* Dense elementwise steps of the optimizers `compile` accepts besides Adam (models/meta_basemodel.py:612-640: torch.optim.SGD
 * lr 0.01, Adagrad lr 0.01 eps 1e-10, RMSprop lr 0.01 alpha 0.99 eps 1e-8), over n floats with the dense gradient g:
 *   SATRANS_OPT_SGD      p -= lr g
 *   SATRANS_OPT_ADAGRAD  s += g^2 ; p -= lr g / (sqrt(s) + eps)
 *   SATRANS_OPT_RMSPROP  s = alpha s + (1 - alpha) g^2 ; p -= lr g / (sqrt(s) + eps)
 * Used with the dense table gradient of satrans_embed_grad_dense (every row: gathered rows + 2 l2 p), i.e. the reference's
 * dense semantics as one sweep over the tables per step; Adam has the lazy-exact kernels above instead. */
#define SATRANS_OPT_SGD 1
#define SATRANS_OPT_ADAGRAD 2
#define SATRANS_OPT_RMSPROP 3
int satrans_optim_flat(int kind, float* p, const float* g, float* state, int64_t n, float lr, float alpha, float eps, void* stream);
int64_t satrans_head_scratch_floats(int B, int FD, int n_dense);

/* ------------------------------------------------------------------------------------------------
 * Optimizer: torch.optim.Adam semantics (reference main.py:343) with the L2 regulariser of
 * meta_basemodel.py:577-593 folded in as its gradient 2*l2*p.
 * ---------------------------------------------------------------------------------------------- */
#define SATRANS_ADAM_EXACT 0   /* torch.optim.Adam's fp32 operations bit for bit (correctly rounded sqrt and divisions) */
#define SATRANS_ADAM_FAST  1   /* hardware sqrt / reciprocal: each update within 3.2e-7 relative of the exact one, ~2.5x fewer
                                  instructions; every kernel form (streaming, gathered rows, lazy replay / flush) runs the
                                  SAME sequence, so the forms still agree bit for bit with each other */
typedef struct satrans_adam_hparams {
    float lr_over_bc1;  /* lr / (1 - beta1^t)                */
    float bc2_sqrt;     /* sqrt(1 - beta2^t)                 */
    float beta1, beta2, eps;
    float l2;           /* l2_reg_embedding (0 for flat dense parameters) */
    int32_t arith;      /* SATRANS_ADAM_EXACT / SATRANS_ADAM_FAST (ABI 6) */
} satrans_adam_hparams;

/* Flat parameter vector (everything that is not an embedding table): p,g,m,v [n]. */
int satrans_adam_flat(float* p, const float* g, float* m, float* v, int64_t n,
                      const satrans_adam_hparams* h, void* stream);
/* the same, and out[0] += sum(vals[0..count)) in fixed order, in one launch (the step's regulariser partial sums) */
int satrans_adam_flat_sum(float* p, const float* g, float* m, float* v, int64_t n, const satrans_adam_hparams* h,
                          const double* vals, int64_t count, double* out, void* stream);

/* Embedding-gradient pipeline over n = (ranks*)B*F gathered rows.
 *   rows [n] int32 arena rows, gemb [n, D] gradient of every gathered row.
 * step 1 (sort):   sorted_rows[n], src[n] = stable sort of rows with their positions;
 *                  touched bitmap [ceil(total_rows/32)] uint32 is cleared and rebuilt (pass NULL to skip it: only
 *                  step 3 reads it).
 * step 2 (touched rows): per distinct row r: g = (sum of its gemb rows in position order) + 2*l2*p[r];
 *                  Adam on arena/m/v row r.
 * step 3 (untouched rows): every row whose bit is clear gets g = 2*l2*p (the reference's dense Adam
 *                  moves EVERY row EVERY step because of the dense regulariser gradient).
 * reg_partials [satrans_embed_reg_partials(total_rows, n, D)] doubles: per-block sums of l2*p^2 over the
 * pre-update values (reference `reg_loss`), filled by step 2 and 3 into disjoint slots.
 */
int64_t satrans_embed_sort_workspace_bytes(int64_t n, int64_t total_rows);
/* positions: optional [n] int32 with positions[i] = i kept by the caller (saves the launch that would write it) */
int satrans_embed_sort(const int32_t* rows, int64_t n, int64_t total_rows, int32_t* sorted_rows,
                       int32_t* src, uint32_t* touched, void* workspace, int64_t workspace_bytes,
                       const int32_t* positions, void* stream);
/* The same sort for the rows of one batch, rows [B, F] (position = b*F + f), when every field has a table of its own: one launch,
 * one workgroup per field sorting in LDS.  seg_field / seg_lo / seg_rows are HOST arrays of F entries: the fields in arena order
 * with the first arena row and the row count of their tables (pairwise disjoint, ascending).  B <= 8192, F <= 64, otherwise
 * SATRANS_E_UNSUPPORTED.  Output identical to satrans_embed_sort's. */
int satrans_embed_sort_fields(const int32_t* rows, int B, int F, const int32_t* seg_field, const int32_t* seg_lo,
                              const int32_t* seg_rows, int32_t* sorted_rows, int32_t* src, void* stream);
/* ... and with the ids -> rows translation of satrans_gather_fwd(out = NULL, rows_out = rows) in the same launch (meta_basemodel.py:
 * 533-535, the lookup's index arithmetic): `rows` [B, F] is an OUTPUT; X / id_dtype / x_stride / cols / row_span / status as for
 * satrans_gather_fwd (an id outside its table sets bit 0 of *status and is recorded as the table's first row); seg_lo[k] must be
 * row_span[2 * seg_field[k]]. */
int satrans_embed_rows_sort_fields(const void* X, int id_dtype, int64_t x_stride, const int32_t* cols, const int64_t* row_span,
                                   int32_t* rows, int B, int F, const int32_t* seg_field, const int32_t* seg_lo,
                                   const int32_t* seg_rows, int32_t* sorted_rows, int32_t* src, int32_t* status, void* stream);
/* The same sort when `ids` [n] is W sorted runs back to back (owner form of the data-parallel step: what W ranks sent an owner;
 * each run ascending, equal rows in position order): ONE launch, every element ranks itself by W - 1 binary searches.  h_run_start:
 * HOST array of W + 1 boundaries (h_run_start[0] = 0, h_run_start[W] = n), W <= 64.  Output identical to
 * satrans_embed_sort(ids, positions = 0..n-1): src[j] = the index in `ids` of sorted element j. */
int satrans_embed_merge_runs(const int32_t* ids, int64_t n, const int64_t* h_run_start, int W, int32_t* sorted_rows, int32_t* src,
                             void* stream);
/* inv[src[i]] = i for i < n: the inverse of a sort's source positions */
int satrans_embed_inverse_positions(const int32_t* src, int64_t n, int32_t* inv, void* stream);
int64_t satrans_embed_reg_partials(int64_t total_rows, int64_t n, int D);
/* last / t: optional (lazy form): last[row] = t for every row stepped */
int satrans_embed_adam_touched(float* arena, float* m, float* v, int D, const int32_t* sorted_rows,
                               const int32_t* src, int64_t n, const float* gemb, float* partial_ws,
                               const satrans_adam_hparams* h, double* reg_partials, int32_t* last, int t,
                               void* stream);
int64_t satrans_embed_partial_ws_floats(int64_t n, int D);
/* rows [first_row, total_rows) that are not in the bitmap; grid_blocks: 0 = the measured optimum (512 persistent blocks
 * of 256 threads), otherwise the grid size to use */
int satrans_embed_adam_untouched(float* arena, float* m, float* v, int64_t first_row, int64_t total_rows, int D,
                                 const uint32_t* touched, const satrans_adam_hparams* h,
                                 double* reg_partials, int grid_blocks, void* stream);
/* touched-row bitmap [ceil(total_rows/32)] of an already sorted id list (cleared first; n may be 0) */
int satrans_embed_mark_touched(const int32_t* sorted_rows, int64_t n, int64_t total_rows, uint32_t* touched,
                               void* stream);

/* Small tables (the caller places them first in the arena): their gradient is a DENSE buffer g_rows [rows, D] - the
 * ordered segmented sums of satrans_embed_segment_sums over the sorted positions that fall into those tables, stored
 * instead of applied (rows nobody gathered keep the zeros the caller wrote) - which data-parallel ranks all-reduce, and
 * satrans_embed_adam_rows then steps EVERY row of [row0, row0+rows) with g = g_rows + 2*l2*p (for an ungathered row that
 * is exactly the reference's regulariser-only step) and sets last[row] = t when `last` is given.
 * Workspaces as for satrans_embed_adam_touched; reg_partials of adam_rows: satrans_embed_adam_rows_partials doubles.
 * satrans_embed_pack_rows: out[j] = gemb[src[j]], the gradient rows of a sorted id list in sorted order (what a rank
 * contributes to the all-gather of the large tables' gradient rows). */
int satrans_embed_segment_sums(const int32_t* sorted_rows, const int32_t* src, int64_t n, const float* gemb, int D,
                               float* partial_ws, double* reg_partials, float* g_rows, void* stream);
int64_t satrans_embed_adam_rows_partials(int64_t rows, int D);
int satrans_embed_adam_rows(float* arena, float* m, float* v, int32_t* last, int64_t row0, int64_t rows, int D,
                            const float* g_rows, const satrans_adam_hparams* h, int t, double* reg_partials,
                            void* stream);
int satrans_embed_pack_rows(const int32_t* src, int64_t n, const float* gemb, int D, float* out, void* stream);

/* Lazy-exact form of the dense step (same tables bit for bit, HBM traffic only for touched rows): instead of
 * satrans_embed_adam_untouched every step, the regulariser-only Adam steps of a row are postponed and replayed with
 * identical arithmetic when the row is next gathered (replay, over the distinct rows of the sorted ids, BEFORE the
 * gather of that step) or for all rows (flush: epoch end, before predict / state_dict).
 *   last   [total_rows] int32: last step applied to each row (0 initially)
 *   table  [>= target+1][2] fp64: table[s] = (fp32(lr / (1 - beta1^s)), 1 / (double)fp32(sqrt(1 - beta2^s))), filled by
 *          the host (the kernels divide by the per-step constant through its double reciprocal, exactly: embed_adam.hip)
 *   h      beta1, beta2, eps, l2 (lr_over_bc1 / bc2_sqrt are ignored)
 *   reg_partials [satrans_embed_lazy_reg_partials(n, D)] doubles (zero-initialised by the caller): per-block sums of
 *          l2*p^2 over the replayed steps; replay writes the first ceil(n*D/256) slots, flush the 4096 after them.
 * satrans_embed_lazy_mark sets last[r] = t for the distinct rows of a step after their Adam update. */
int64_t satrans_embed_lazy_reg_partials(int64_t n, int D);
int satrans_embed_lazy_replay(float* arena, float* m, float* v, int32_t* last, int D, const int32_t* sorted_rows,
                              int64_t n, int target, const double* table, const satrans_adam_hparams* h,
                              double* reg_partials, void* stream);
int satrans_embed_lazy_flush(float* arena, float* m, float* v, int32_t* last, int64_t total_rows, int D, int target,
                             const double* table, const satrans_adam_hparams* h, int64_t n, double* reg_partials,
                             void* stream);
/* The same two calls with the partial sums of the regulariser in the step kernels' arithmetic: every replayed step adds
 * l2 * p^2 with p widened to double first (as satrans_embed_adam_touched / _untouched do), where the two calls above add an
 * element's postponed p^2 in fp32 and widen once.  arena, m, v and last come out the same bits; a caller that holds ONE total of
 * the step and replay sums against the streaming form's (optim.TableAdam(track_regularizer=True)) uses these.  One loop per
 * lane over the per-step table: slower than the calls above where many steps are pending. */
int satrans_embed_lazy_replay_reg64(float* arena, float* m, float* v, int32_t* last, int D, const int32_t* sorted_rows,
                                    int64_t n, int target, const double* table, const satrans_adam_hparams* h,
                                    double* reg_partials, void* stream);
int satrans_embed_lazy_flush_reg64(float* arena, float* m, float* v, int32_t* last, int64_t total_rows, int D, int target,
                                   const double* table, const satrans_adam_hparams* h, int64_t n, double* reg_partials,
                                   void* stream);
int satrans_embed_lazy_mark(const int32_t* sorted_rows, int64_t n, int32_t* last, int t, void* stream);

/* The lazy form for 1-wide tables (LinearModel's arena [arena_rows, 1]; additive under ABI 7): the bits of
 * satrans_adam_flat(h.l2) over a dense gradient buffer that is zero for every row nobody gathered, at touched-rows cost.
 *   last, table, h   as above (replay and flush take lr_over_bc1 / bc2_sqrt of step s from table[s])
 * satrans_embed1_lazy_replay: every slot row of a batch to step `target`, BEFORE satrans_linear_fwd reads it.  The rows are
 *   `rows` [n] when given (any order, duplicates allowed, rows outside the arena skipped), otherwise those of X [B, x_stride]
 *   through `fields` (F fields, R slots: satrans_linear_fwd's index arithmetic - every slot of a list, an id outside its table
 *   counts as the table's first row).  Duplicates are settled by an integer atomic maximum on last[row]: no sort, and the
 *   result does not depend on which lane wins.
 * satrans_embed1_adam_rows: step t of the distinct rows of a sorted list with g[row] + 2 l2 p, then last[row] = t and
 *   g[row] = 0 - `g` [arena_rows] is the buffer satrans_linear_bwd stored its sums in, and is all-zero again afterwards.
 * satrans_embed1_lazy_flush: every row to step `target`. */
int satrans_embed1_lazy_replay(float* arena, float* m, float* v, int32_t* last, int64_t arena_rows, const int32_t* rows,
                               int64_t n, const satrans_pool_field* fields, int F, int R, const void* X, int id_dtype,
                               int64_t x_stride, int B, int target, const double* table, const satrans_adam_hparams* h,
                               void* stream);
int satrans_embed1_adam_rows(float* arena, float* m, float* v, int32_t* last, float* g, int64_t arena_rows,
                             const int32_t* sorted_rows, int64_t n, const satrans_adam_hparams* h, int t, void* stream);
int satrans_embed1_lazy_flush(float* arena, float* m, float* v, int32_t* last, int64_t arena_rows, int target,
                              const double* table, const satrans_adam_hparams* h, void* stream);

/* Diagnostic behind the replay's arithmetic.  Replay and flush run four elements per lane on the packed fp32 pipe with the
 * square root and the division written out as correctly rounded fma sequences (embed_adam.hip); this call counts the results
 * that differ from the IEEE operations: mode 0 = square root over the floats with bit patterns [first, first + count),
 * restricted to the operand range of the packed path; mode 1 = division over `count` pseudo-random pairs (seed `first`) of that
 * range; mode 2 / 3 = the same two operations BELOW that range through their exact power-of-two scaling (every positive float
 * under 2^-100, subnormals included; numerators from the smallest subnormal to 2^-80 and signed zeros).  *mismatches is HOST
 * memory.  Used by tests/test_gpu_parity.py (every float of the range for modes 0 and 2). */
int satrans_debug_check_packed_math(int mode, uint64_t first, uint64_t count, uint64_t* mismatches, void* stream);

/* Dense materialisation of the embedding gradient (debug / parity tests only):
 * g_arena [total_rows, D] += scatter of gemb by rows (position order), + 2*l2*p when l2 != 0. */
int satrans_embed_grad_dense(const float* arena, const int32_t* sorted_rows, const int32_t* src, int64_t n,
                             const float* gemb, int64_t total_rows, int D, float l2, float* g_arena,
                             void* stream);

/* Sum of `count` doubles in index order -> out[0] (+= when accumulate != 0). */
int satrans_sum_f64(const double* v, int64_t count, double* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scenario-specific attention maps: predict's `showattn` branch (reference models/meta_basemodel.py:421-426, 439-458,
 * 506-514), the per-(scenario, label class) sums of a layer's `normalized_att_scores` over the samples of a batch.
 *   att   [H, B, F, F] one layer's attention in the caller's sample order, as satrans_layer_fwd / satrans_layer_fwd_generic
 *         write it
 *   key   [B] int32: the accumulator row of every sample, 3 j + c for scenario j and class c (0: label 1, 1: label 0, 2: any
 *         other label), or -1 for a sample that counts nowhere (a key outside [-1, K) counts nowhere too)
 *   acc   [K, H, F, F] fp64, K = 3 S, ACCUMULATED: acc[k] += the sum of att[:, b] over the samples b with key[b] == k
 * Deterministic: no float atomics; a stable grouping of the samples by scenario, fixed blocks of 128 sample positions per
 * scenario summed in fp64 (one sum per class), the block sums folded in a fixed order.  The partition depends on B, the scenario
 * counts and the shape only, so two calls on the same inputs give the same bits.  Any F, odd F included.  workspace:
 * satrans_attn_stats_workspace_bytes(B, H, F, K) bytes (-1 on bad sizes, K not a multiple of 3 included). */
int64_t satrans_attn_stats_workspace_bytes(int B, int H, int F, int K);
int satrans_attn_stats_accumulate(const float* att, const int32_t* key, int B, int H, int F, int K, double* acc,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Instance-level attention search: predict's `inst_attn_dict` and `instattn` branches (reference models/meta_basemodel.py:
 * 440-445, 460-499).  The (sample, head) pairs of a batch whose map of one layer satisfies a rule are found on the device and only
 * their maps, probabilities and input rows are copied out.  Added under ABI 7: new entry points and new struct types only.
 *
 * A rule is a conjunction of 1..8 clauses, a clause a disjunction of 1..4 atoms, an atom `att[h, b, q, k] > thr`: strict, in
 * fp32, never true for a NaN.  The reference's second rule, `A and (B or C)`, is two clauses of one and two atoms. */
#define SATRANS_ATTN_MAX_RULES 8
#define SATRANS_ATTN_MAX_CLAUSES 8
#define SATRANS_ATTN_MAX_ATOMS 4
#define SATRANS_ATTN_MAX_HEADS 16

typedef struct {
    int32_t q, k; /* query and key field, both in [0, F) */
    float thr;    /* finite */
} satrans_attn_atom;

typedef struct {
    int32_t n_clauses;                         /* 1..SATRANS_ATTN_MAX_CLAUSES */
    int32_t n_atoms[SATRANS_ATTN_MAX_CLAUSES]; /* 1..SATRANS_ATTN_MAX_ATOMS for the clauses in use */
    satrans_attn_atom atoms[SATRANS_ATTN_MAX_CLAUSES][SATRANS_ATTN_MAX_ATOMS];
} satrans_attn_rule;

typedef struct {
    int64_t index; /* global sample index: first_index + the sample's position in its batch */
    int32_t head;
    int32_t rule; /* the rule that matched (the caller's choice, e.g. -1, in a hand-built list) */
} satrans_attn_match;

/* satrans_attn_inst_match: append one record per (sample b, head h, rule r) with rule r true on att[h, b] to a device list.
 *   att      [H, B, F, F] one layer's attention as satrans_layer_fwd / satrans_layer_fwd_generic write it
 *   rules    HOST array of n_rules (1..8) rules, copied by value into the launch; validated here (fields in [0, F), finite
 *            thresholds, counts within bounds): a bad rule is SATRANS_E_BADARG, never a device fault
 *   eligible optional [B] uint8: bit r set = rule r may match sample b (0: the sample matches nothing, 0xff: every rule may;
 *            NULL: all of them) - label and column filters, evaluated by the caller
 *   records  the list, `capacity` entries in all; total [1] int64 on the device = the records found so far, by this and earlier
 *            calls.  The call appends at position total[0] while that is below `capacity` (the capacity left is capacity -
 *            total[0], taken on the device: no host read between batches) and advances total[0] by EVERY match, beyond the
 *            capacity too: total[0] > capacity afterwards means the list is truncated, and total[0] stays exact.
 *   range    optional [2] int64 on the device: the list positions this call filled, clamped to the capacity
 * Order within a call: sample, then head, then rule - with first_index = the batch's offset the list of a pass does not depend
 * on the batch size.  (Deviation: the reference loops head-major inside each batch.)  Deterministic: one lane per pair, per-wave
 * counts, one workgroup scans them, records written at the scanned offsets; no atomics.  A lane reads only the atoms its rules
 * name (short-circuit).  Any F (odd included), any B, H in 1..16, B * H < 2^28.
 *
 * satrans_attn_inst_gather: for the records m of [m0, m1) (intersected with range[0..2) when `range`, a device pointer, is
 * given) whose index lies in [first_index, first_index + B): maps[m] = att[head, index - first_index] (F * F dwords, bit for bit),
 * pred[m] = prob[index - first_index], x_rows[m] = the first row_dwords dwords of row index - first_index of x (rows
 * x_stride_dwords apart; any id dtype).  maps, pred and x_rows are each optional and indexed by LIST position.  Records of other
 * batches or with a head outside [0, H) are skipped.  The same call serves hand-built lists (every head of chosen samples).
 *
 * workspace of _match: satrans_attn_inst_workspace_bytes(B, H, F) bytes (-1 on bad sizes).  satrans_attn_inst_check_rules runs
 * the validation alone (no device). */
int64_t satrans_attn_inst_workspace_bytes(int B, int H, int F);
int satrans_attn_inst_check_rules(const satrans_attn_rule* rules, int n_rules, int F);
int satrans_attn_inst_match(const float* att, int B, int H, int F, const satrans_attn_rule* rules, int n_rules,
                            const uint8_t* eligible, int64_t first_index, satrans_attn_match* records, int64_t capacity,
                            int64_t* total, int64_t* range, void* workspace, int64_t workspace_bytes, void* stream);
int satrans_attn_inst_gather(const float* att, int B, int H, int F, const satrans_attn_match* records, int64_t m0, int64_t m1,
                             const int64_t* range, int64_t first_index, float* maps, const float* prob, float* pred,
                             const void* x, int64_t x_stride_dwords, int row_dwords, void* x_rows, void* stream);

/* The per-step training metrics of fit(verbose > 0) (meta_basemodel.py:330-337: sklearn log_loss and roc_auc_score on host
 * copies of every batch) for one batch in one launch: out[0] = log_loss(y, p.astype(float64)) (probabilities clipped to
 * [eps, 1 - eps] with the fp64 eps, mean), out[1] = roc_auc_score(y, p) (tied scores count one half; NaN when only one class
 * is present).  y, p: [n] fp32, n <= 8192; out: two doubles in device memory.  Fixed summation order. */
int satrans_batch_metrics(const float* y, const float* p, int n, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATRANS_HIP_H */
