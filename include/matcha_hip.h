/*
 * matcha_hip.h -- C ABI of the MI355X (gfx950) hot path of MATCHA's hyperedge-classifier
 * training loop.  One shared library, libmatcha_hip.so; plain pointers and sizes only.
 *
 * Conventions
 *   - every buffer is a caller-owned DEVICE pointer (hipMalloc / torch .data_ptr()), contiguous,
 *     row-major; fp32 data, int64 node ids at the boundary (the reference's dtype, main.py:433);
 *   - no allocation, no ownership transfer, no hidden synchronisation: every call enqueues work
 *     on `stream` (a hipStream_t passed as void*) and returns; scratch comes from the caller via
 *     matcha_workspace_bytes();
 *   - return 0 on success, a negative errno-style code otherwise; matcha_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - reentrant across streams; one process per GPU.
 *
 * The reference (ma-compbio/MATCHA, Code/) is pure Python/PyTorch and has no FFI of its own; each
 * entry point cites the reference lines whose ATen call sites it replaces.  The reference-side
 * binding (a ctypes stub for Code/Modules.py) is in INTEGRATION.md.
 */
#ifndef MATCHA_HIP_H
#define MATCHA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MATCHA_ABI_VERSION 7

#define MATCHA_OK 0
#define MATCHA_EINVAL (-22) /* bad argument (shape, alignment, null pointer) */
#define MATCHA_EHIP (-5)    /* a HIP runtime call or kernel launch failed    */
#define MATCHA_ENOMEM (-12) /* workspace too small                             */

#define MATCHA_MAX_L 8      /* widest hyperedge (BASELINE.json configs[4]: k in 2..8) */
#define MATCHA_MAX_LONG_L 32 /* widest row of the long forward (matcha_forward_long), of matcha_get_embedding_long and of the long training pair (matcha_forward_long_train, matcha_backward_long) */
#define MATCHA_N_HEAD 8     /* main.py:616 */

typedef void* matcha_stream_t; /* hipStream_t */

int matcha_abi_version(void);
const char* matcha_last_error(void);
/* number of visible HIP devices (0 on a CPU-only box; never fails) */
int matcha_device_count(void);

/* Optional live timing of ONE kernel class with HIP events recorded on the launch stream (used by bench.py
 * for the roofline of the dominant kernel, inside the timed region).  select(0) switches it off.  read()
 * synchronises on the recorded events and returns the summed duration [ms], the number of launches and the
 * summed algorithmic work (FLOP for the GEMM classes, bytes otherwise), then clears the accumulators.
 * Process-global, single-threaded use; do not use while a stream capture is active. */
#define MATCHA_PROF_GEMM_NT 1
#define MATCHA_PROF_GEMM_NN 2
#define MATCHA_PROF_GEMM_TN 3
#define MATCHA_PROF_ATTN_FWD 4
#define MATCHA_PROF_ATTN_BWD 5
#define MATCHA_PROF_EMBED_FWD 6
#define MATCHA_PROF_EMBED_SCATTER 7
#define MATCHA_PROF_LN3_FWD 8
#define MATCHA_PROF_LN3_BWD 9
#define MATCHA_PROF_HEAD_FWD 10
#define MATCHA_PROF_HEAD_BWD 11
#define MATCHA_PROF_ADAMW 12
#define MATCHA_PROF_NEG_SAMPLE 13
#define MATCHA_PROF_ADJ_ENCODE 14
#define MATCHA_PROF_GATHER_ROWS 15
#define MATCHA_PROF_FUSED_FWD 16
#define MATCHA_PROF_FUSED_BWD 17
#define MATCHA_PROF_FRONT_FWD 18   /* gather + attribute_nn + next_w + tanh (front_fused.hip) */
#define MATCHA_PROF_FRONT_BWD 19   /* LayerNorm backward of the d x_hat partials + next_w / attribute_nn backward + scatter */
#define MATCHA_PROF_ADJ_RECON 20   /* adj front end: reconstruction branch, forward (+ its backward in a training forward); FLOP       */
#define MATCHA_PROF_ADJ_BWD 21     /* adj front end: encoder backward (dW1, dZ, dW0); FLOP.  MATCHA_PROF_ADJ_ENCODE (14) = the fused
                                      forward (gather-GEMM, W1, attribute path, next_w); FLOP.  The adj classes count the EXPECTED work
                                      of uniformly drawn node ids: a token's feature row has sum_i n_i^2 / N columns on average         */
int matcha_profile_select(int32_t kernel_class);
int matcha_profile_read(double* total_ms, int64_t* launches, double* work);

/* Launch log (ABI 7): which kernels did a call run?  matcha_launch_log(1) clears the log and starts counting every kernel launch the
 * library makes (by the kernel's name, template instances together), matcha_launch_log(0) stops; matcha_launch_log_read writes one
 * "kernel_name count\n" line per kernel seen (MATCHA_ENOMEM if `cap` is too small).  The parity tests assert the kernel set with
 * it: the library picks kernels by batch size and embed_dim, and a test that is "about" a kernel must fail when a size rule moves
 * it onto another one.  A captured graph counts at capture time, not per replay.  Process-global, single-threaded use. */
int matcha_launch_log(int32_t on);
int matcha_launch_log_read(char* out, size_t cap);

/* Route record: which kernel route did the last forward that a backward may follow take on workspace `ws`?  Writes one "field value\n"
 * line per field of the record the backward replays (0 / 1; `fwd_values`: where the embed_dim-64 large-batch forward took the heads'
 * value rows y_h = M_h x_hat from -- 1 a product per token inside the kernel, 2 a product per token on the node route with the r rows
 * gathered, 3 gathered from the per-node value table, 0 another kernel ran the forward).  MATCHA_EINVAL when no forward is on record
 * (none ran, it kept nothing, or a backward consumed it), MATCHA_ENOMEM if `cap` is too small.  Host state only: no launch, no sync. */
int matcha_route_read(const void* ws, char* out, size_t cap);

/* A/B switches for tests and profiling.  Each option is read from the environment variable MATCHA_<NAME> (upper case) ONCE,
 * when the library is loaded, and can be changed afterwards only through matcha_set_option -- no entry point reads the
 * environment per call.  NINE switches: "disable_fused" (1 = layer-by-layer kernels at every embed_dim, also instead of the fused
 * attention block of embed_dim 128; 2 = only the front end as separate kernels, the encoder stays fused), "disable_merged" (the reference's four products per attention head instead of the
 * merged two; they live on the layer-by-layer kernels, so at embed_dim 64 this implies disable_fused), "disable_small_batch" (the
 * large-batch forward and plan kernels at every size), "disable_wide_gemm" (embed_dim >= 128: the 64-wide GEMM / attention kernels
 * instead of the 128 x 128 ones), "disable_node_front" (the table front end once per TOKEN at every size: without it, a step at embed_dim 64
 * whose token capacity B L + 1 is at least 4 (n_nodes + 1) -- large-batch kernels, not deterministic, no row-sparse table gradient --
 * computes x0, X and the front end's backward once per NODE and gathers the rows by node id; same logits and losses bit for bit, the
 * gradients differ in summation order only), "disable_node_r" (on the node route: the heads' r rows r = B_h x_hat + b_h computed per TOKEN inside
 * the forward kernel and handed to the backward in the per-half-tile record; without it node_r_kernel computes them once per (node, head)
 * and both encoder kernels gather them by node id -- same logits and losses bit for bit), "disable_node_v" (on the node route with the r
 * table: the backward forms dZ = dDyn M_h and Z per token; without it a differentiated forward also leaves y = M_h x_hat per (node, head) and
 * the backward gathers the rows, from a token capacity of 64 (n_nodes + 1) on -- forward outputs bit for bit the same, gradients equal to
 * rounding), "disable_node_dx" (on the node route with the value table: the encoder's input gradients -- d x_hat of the eight heads, the
 * static branch's dXs -- are left per TOKEN and node_scatter_kernel adds them per node in one walk over the tokens; without it both producers
 * add into per-node rows, one replica per head, and node_scatter_kernel finishes each node row -- forward outputs and the encoder's gradients
 * bit for bit the same, the front end's gradients the same sums in another order), "disable_launch_pairs" (the fused embed_dim 64 step with
 * every small launch on its own; without it independent small launches share a launch as block roles: the chain rule's blocks of
 * fbm_chain_kernel un-fold their own rows -- no fb_unfold_kernel --, and on the node route fb_unfold2's vectors ride in node_scatter_kernel, the
 * plan's tile_pack pass in the table front end's forward and its tile_compact pass in node_r_kernel -- four launches fewer per node-route step,
 * one fewer elsewhere; every role runs the text of the stand-alone kernel, so the plan and every output are the same bits either way;
 * matcha_backward follows what the forward recorded), "disable_row_pack" (the fused embed_dim 64 step's ragged plan in batch order; without it
 * the plan's rows are a permutation of the batch's, ordered by size class so that the half tiles fill to 31 tokens -- the loss-in-forward training
 * step and the forward-only call, where the five-launch plan runs (more than 1 024 rows or eight planning superblocks) AND the order's arrays fit
 * the plan regions it borrows: L >= 3 and at least five planning superblocks, i.e. B L >= 8 064 token slots (L = 5: from 1 613 rows); logits and losses are the same bits either way, gradients the same sums in another order;
 * matcha_ragged_plan itself never reorders); development: "debug_nan", "fused_dbg" (bit 0: the backward of
 * pff_n1's convolutions inside the forward kernel at every batch size, instead of tail_bwd64_kernel for large batches).  (Whether the tail's backward runs inside the forward
 * kernel is a per-call choice: matcha_step_opts.loss_in_forward.)  Returns MATCHA_EINVAL for an unknown name;
 * matcha_get_option returns -1 for one.
 * Process-global: flip them only while no call is in flight. */
int matcha_set_option(const char* name, int32_t value);
int32_t matcha_get_option(const char* name);

/* Device-side status word of the entry points that index memory by node id.  `status` is a caller-owned DEVICE int32[4],
 * zeroed by the caller; kernels OR / add into it and the caller inspects it whenever it synchronises anyway (no entry point
 * syncs).  Ids that would index out of bounds are replaced by 0 (the padding id) so that no kernel reads or writes outside
 * its buffers; the reference raises IndexError there (nn.Embedding, Modules.py:34/:67).
 *   status[0]  bit 0: a node id of x / ids was outside [0, n_nodes];  bit 1: the sampler met a node without a chromosome
 *              (node2chrom < 0 or >= n_chrom) and kept it unchanged
 *   status[1]  number of negatives whose 65 536 trials were exhausted (the row is returned equal to its positive; the
 *              reference would loop forever, main.py:392)
 *   status[2..3] reserved */
#define MATCHA_STATUS_BAD_ID 1
#define MATCHA_STATUS_BAD_CHROM 2

/* ------------------------------------------------------------------------------------------
 * Model description: shapes + one pointer per LIVE tensor of the reference's
 * Classifier.state_dict() (Modules.py:204-249).  The same struct type carries parameters
 * (`matcha_tensors` of weights) and gradients (`matcha_tensors` of grads; same shapes).
 * Dead tensors of the reference (encode2.*, fc2, pff_n2, decoder biases, node_embedding.next_w;
 * SURVEY.md headline fact 3) are never read and have no slot.
 * ------------------------------------------------------------------------------------------ */
typedef struct matcha_shape {
  int32_t d;        /* embed_dim = d_model = d_k = d_v = bottle_neck (main.py:517); multiple of 16, <= 256 */
  int32_t n_attr;   /* C+1 columns of the attribute table (main.py:497-512) */
  int32_t n_nodes;  /* N; node ids are 1..N, 0 = padding */
  int32_t n_chrom;  /* C (adj mode); may be 0 in table mode */
  int32_t mode;     /* 0 = table (Wrap_Embedding, Modules.py:29-34); 1 = adj (MultipleEmbedding :125-201) */
  int32_t max_bins; /* adj: max_i n_i */
} matcha_shape;

typedef struct matcha_tensors {
  /* front end -- table mode */
  float* table;      /* [N+1, d]       node_embedding.weight                                    */
  /* front end -- adj mode: per-chromosome tensors packed back to back, chromosome i at bounds[i] */
  float* adj_w0;     /* sum_i [d, n_i] node_embedding.Embedding_Linear{i}."tied weight_0"; offset d*bounds[i] */
  float* adj_w1;     /* [C, d, d]      node_embedding.Embedding_Linear{i}."tied weight_1"         */
  float* recon_w;    /* sum_i [n_i, d] node_embedding.Embedding_recon{i}.FF_Linear0.weight; offset d*bounds[i] */
  float* recon_b;    /* [N]            node_embedding.Embedding_recon{i}.FF_Linear0.bias; offset bounds[i]     */
  /* attribute path (Modules.py:243-249, :263-264) */
  float* attr_w;     /* [d, n_attr]    attribute_nn.weight */
  float* attr_b;     /* [d]            attribute_nn.bias   */
  float* next_w;     /* [d, d]         next_w.FF_Linear0.weight (Modules.py:270) */
  float* next_b;     /* [d] */
  /* encode1.mul_head_attn (Modules.py:463-575) */
  float* ln_q_g; float* ln_q_b;   /* layer_norm1 */
  float* ln_k_g; float* ln_k_b;   /* layer_norm2 */
  float* ln_v_g; float* ln_v_b;   /* layer_norm3 */
  float* w_q;        /* [8d, d] w_qs.weight */
  float* w_k;        /* [8d, d] w_ks.weight */
  float* w_v;        /* [8d, d] w_vs.weight */
  float* fc1_w;      /* [d, 8d] fc1.weight  */
  float* fc1_b;      /* [d] */
  /* encode1.pff_n1 (Modules.py:604-605, :353-376); Conv1d(k=1) weight [d,d,1] == [d,d] */
  float* pff0_w; float* pff0_b;
  float* pff1_w; float* pff1_b;
  float* pff_ln_g; float* pff_ln_b;
  /* Classifier tail (Modules.py:290-299) */
  float* ln1_g; float* ln1_b;     /* layer_norm1 (dynamic) */
  float* ln2_g; float* ln2_b;     /* layer_norm2 (static)  */
  float* cls_w;      /* [d]  pff_classifier.PWF_Conv0.weight [1,d,1] */
  float* cls_b;      /* [1] */
} matcha_tensors;

/* Frozen (non-trainable) inputs of the front end. */
typedef struct matcha_frozen {
  const float* attr_table;   /* [N+1, n_attr] attribute_dict_embedding.weight, row 0 zeros (main.py:508) */
  const int32_t* bounds;     /* [C+1] Modules.py:138 num_list = [0, n_0, n_0+n_1, ...] (adj; device)     */
  const float* feats;        /* adj: sum_i [n_i, n_i] feature matrices (main.py:571-577), chrom i at feat_off[i] */
  const int64_t* feat_off;   /* [C+1] element offsets into feats (device)                                 */
  const float* inter;        /* adj: [N, N] z-scored inter-chromosome matrix (Modules.py:146-154)         */
  const int32_t* bounds_host;/* [C+1] same as bounds, HOST pointer                                         */
  /* ---- ABI 6 (all zero = the layouts above) ---- */
  int32_t feat_row_pad;      /* adj: 0 = the rows of chromosome i are n_i floats, back to back; P > 0 (a multiple of 4) = every row is
                                padded with zeros to a multiple of P floats, `feats` is 16-byte aligned and every feat_off[i] a
                                multiple of 4 -- aligned 16-byte loads of feature rows; the fused embed_dim-64 kernels
                                (csrc/adj_fused.hip) require P = 64, other values run the layer-by-layer kernels               */
  int32_t attr_mode;         /* 0 = attribute rows are read from attr_table; 1 = the table has the structure main.py:497-512 builds
                                (one-hot chromosome || bin index inside the chromosome / attr_scale, row 0 zeros; the caller has
                                verified it bit for bit) and kernels MAY rebuild a token's row from its node id, attr_bounds and
                                attr_scale instead of reading it (one random row per token instead of two).  Not every kernel
                                rebuilds: at embed_dim 64 the fused forward does, while the fused front end's backward and the
                                layer-by-layer attribute_nn backward gather attr_table.  So attr_table is to be given under
                                attr_mode 1 as well: the fused embed_dim-64 front end (forward and backward) and every
                                layer-by-layer backward return MATCHA_EINVAL without it; only forward calls that run
                                embed_fwd_kernel or the fused adj forward do without.  Its CONTENTS must equal the rows computed
                                from attr_bounds and attr_scale -- all three derived from one snapshot of the table -- or the
                                forward and the backward of one step read different attribute rows                            */
  int32_t attr_ld;           /* attr_mode 0: row stride of attr_table in floats (0 = n_attr); 32 = rows padded to one 128-byte
                                fetch unit                                                                                       */
  float attr_scale;          /* attr_mode 1: num[0] of main.py:503                                                               */
  const int32_t* attr_bounds;/* attr_mode 1: device int32 [n_attr] = 0, n_0, n_0+n_1, ..., N                                      */
} matcha_frozen;

/* Per-call options of the fused step. */
typedef struct matcha_step_opts {
  int32_t training;          /* 0: eval (no dropout); 1: train (dropout with the seeds below)            */
  int32_t random_chrom;      /* adj: the chromosome drawn at Modules.py:192 (caller draws it)             */
  float p_drop_adj;          /* Modules.py:174  (0.2) */
  float p_drop_fc1;          /* Modules.py:226  (0.3) */
  float p_drop_pff;          /* Modules.py:227  (0.4) */
  float alpha;               /* main.py:166 loss = bce*alpha + recon*beta */
  float beta;
  const uint64_t* seed;      /* DEVICE pointer to the 64-bit dropout seed of this step (graph-replay safe) */
  int32_t forward_only;      /* 1: matcha_backward will NOT be called on this workspace (inference / no_grad): the
                                forward may keep every intermediate on chip (fused kernel) and save nothing          */
  int32_t loss_in_forward;   /* 1 (training step with y, w given; embed_dim 64): matcha_forward also runs the backward of the
                                classifier tail for loss = alpha*bce (+ beta*recon) and keeps the result in the workspace;
                                matcha_backward must then be called with the SAME opts and dlogits == NULL.  0: the
                                backward pass starts from the saved activations (required for an arbitrary dlogits)   */
  int32_t* status;           /* optional DEVICE int32[4] status word (see above); NULL = not reported                   */
  int32_t sparse_table_grad; /* table mode, matcha_backward: 1 = do NOT add the table gradient into grads->table; leave it as a
                                per-token (node id, gradient row) list in the workspace for matcha_table_grad_rows (the
                                row-sparse data-parallel exchange); 0 = dense grads->table as usual      */
  int32_t deterministic;     /* table mode, matcha_backward: 1 = the embedding backward sorts the tokens by node id and adds each
                                node's rows in token order with ONE writer per table row (csrc/table_grad.hip: bitwise
                                reproducible, ~60 us per 65 536-row step at hg38 1 Mb sizes); 0 = float atomics from the
                                front-end backward kernel (order of additions varies from run to run, like
                                torch.nn.Embedding's CUDA backward; nothing else in the step is order-dependent)            */
  void* encoder_done_event;  /* optional hipEvent_t (NULL = off): matcha_backward records it on `stream` as soon as the gradients
                                of every parameter from ln_q_g to cls_b (the encoder, pff_n1 and the classifier tail -- the
                                contiguous tail of a flat gradient buffer laid out in matcha_tensors order) are final, i.e.
                                before the front-end backward and the embedding scatter run: a data-parallel caller starts the
                                all-reduce of that part on a second stream and overlaps it with the rest of the backward      */
  const int32_t* random_chrom_dev; /* ABI 6, optional (NULL = use random_chrom): DEVICE int32 holding the chromosome drawn at
                                Modules.py:192, read by the kernels when they run -- a step captured in a hipGraph then replays with a new
                                draw every time the caller rewrites the cell (random_chrom itself is a launch parameter and would be
                                frozen into the graph).  Honoured by the fused adj front end (embed_dim 64, feat_row_pad 64:
                                matcha_random_chrom_dev_supported); other shapes return MATCHA_EINVAL.  Valid range [0, n_chrom): any other
                                value in the cell means "no reconstruction branch" (loss 0, no gradient), like random_chrom = -1   */
} matcha_step_opts;

/* 1 if matcha_forward / matcha_backward honour opts->random_chrom_dev for this shape and these frozen inputs (table mode: always --
 * nothing reads the chromosome there). */
int matcha_random_chrom_dev_supported(const matcha_shape* shp, const matcha_frozen* frozen);

/* Scratch (bytes) the fused forward+backward needs for a [B,L] batch. */
size_t matcha_workspace_bytes(const matcha_shape* shp, int64_t B, int32_t L);
/* Scratch (bytes) that is enough for matcha_forward with opts->forward_only = 1 (inference: predict(), the pairwise sweep,
 * save_embeddings).  At embed_dim 64 only the ragged plan, two [tokens, d] buffers and the front end's buffers exist
 * (~1 KB per token instead of ~20 KB); for other shapes it equals matcha_workspace_bytes. */
size_t matcha_workspace_bytes_forward(const matcha_shape* shp, int64_t B, int32_t L);

/* Classifier.forward(x, return_recon=True) (Modules.py:278-318) + the weighted BCE of main.py:56.
 *   x      int64 [B,L], 0 = padding
 *   y, w   float [B] labels / BCE weights, may be NULL (then no loss is computed)
 *   logits float [B]  (the reference returns [B,1] logits; callers apply sigmoid themselves)
 *   losses float [3]  {bce (mean over B), recon_loss, m = rows the recon mean ran over (0 in table mode)} -- m lets
 *                     data-parallel callers weight each rank's recon gradient by m_rank / m_global
 * Activations needed by matcha_backward stay in `ws`. */
int matcha_forward(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                   const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L,
                   const float* y, const float* w, float* logits, float* losses,
                   void* ws, size_t ws_bytes, matcha_stream_t stream);

/* Long rows: the inference forward for x [B, L] with 2 <= L <= MATCHA_MAX_LONG_L (32), B >= 1, B*L < 2^31 - 2 and at most
 * 65 535 * 128 token rows (the layer-by-layer kernels' launch bound); every shape matcha_forward accepts, both front ends.
 * The entry points without "long" in their name keep MATCHA_MAX_L.  L <= 8 is accepted too, so that the long kernels can be held against
 * matcha_forward on identical input.
 *   opts->training must be 0 and opts->forward_only 1 (anything else: MATCHA_EINVAL before any device call -- dropout and the
 *   backward for long rows do not exist); opts->status and, for the adj front end, opts->random_chrom are honoured as in
 *   matcha_forward (opts->random_chrom_dev: MATCHA_EINVAL).
 *   logits float [B] out;  losses float [3] as matcha_forward (bce unused: slot 0 is not written), may be NULL.
 * Caller-owned memory, asynchronous on `stream`, no allocation, no memset node, no read-back; every refusal before any launch.
 * matcha_workspace_bytes_long is host only and returns 0 (+ matcha_last_error) for a bad argument; the layout is forward-only:
 * 12 d floats per token where embed_dim is a multiple of 64 (merged heads), 28 d otherwise, + 20 B of plan per token and 8 B per row (+ d floats, adj). */
size_t matcha_workspace_bytes_long(const matcha_shape* shp, int64_t B, int32_t L);
int matcha_forward_long(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                        const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L,
                        float* logits, float* losses, void* ws, size_t ws_bytes, matcha_stream_t stream);

/* Long rows: Classifier.get_embedding(x) (Modules.py:261-276) for x [B, L], 2 <= L <= MATCHA_MAX_LONG_L.  The bounds, option rules and
 * refusals of matcha_forward_long (training 0, forward_only 1, no random_chrom_dev, opts->status honoured; L <= 8 accepted so that it can be
 * held against matcha_get_embedding), its workspace (matcha_workspace_bytes_long) and its chain up to pff_n1's convolutions; then
 *   dynamic float [B,L,d], static float [B,L,d] as matcha_get_embedding;
 *   attn    float [8B,L,L], optional (may be NULL): the probabilities in the REFERENCE's layout -- block h*B + b, row = query slot, column =
 *           key slot, both as they stand in x.  The attention kernel (attn_long_prob_kernel) writes every element itself: real query x
 *           real key from its tile, every padding key slot the padding column's probability (one value per query, bitwise equal across its
 *           padding slots), the diagonal 0, rows of padding queries 0, the whole block of an all-padding row 0.  The buffer needs no memset
 *           and nothing runs behind the kernel.  NULL: the plain attn_long_kernel runs, and dynamic / static_ are the same bits either way;
 *   losses  float [3] as matcha_forward_long, may be NULL.
 * A workspace below the query's size is refused as an argument error (MATCHA_EINVAL), like every other refusal before any device call.
 * Caller-owned memory, asynchronous on `stream`, no allocation, no memset node, no read-back.  Not differentiable. */
int matcha_get_embedding_long(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                              const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, float* dynamic,
                              float* static_, float* attn, float* losses, void* ws, size_t ws_bytes, matcha_stream_t stream);

/* Per-locus scores: which locus of a hyperedge does the model support least?  The reference's logit is the masked mean of a per-position
 * score, pff_classifier((layer_norm1(dynamic) - layer_norm2(static))^2) of shape [B, L, 1] (Modules.py:290-311); this entry keeps it.
 * matcha_forward_long's chain up to pff_n1's convolutions, on its workspace (matcha_workspace_bytes_long), with its bounds, option rules and
 * refusals (2 <= L <= 32, training 0, forward_only 1, no random_chrom_dev, opts->status honoured); then head_scores_kernel, which is
 * head_fwd_kernel with the per-token value kept:
 *   scores float [B,L]       the score of the locus in slot l of x[b] (a zero inside a row stays where it stands), exactly 0.0f at padding slots;
 *   logits float [B]         optional (may be NULL): sum of the row's scores / (k + 1e-15) -- the bits matcha_forward_long writes for the same (x, L);
 *   lowest, order            0 <= lowest <= 32; order int64 [B, lowest], NULL iff lowest == 0: order[b][j] = the slot of the j-th lowest score among
 *                            the row's k real loci -- ascending by value, ties to the lower slot, a NaN behind every number --, -1 for j >= k;
 *   losses float [3]         as matcha_forward_long, may be NULL.
 * The kernel writes every element of scores, logits and order itself: the buffers need no memset and nothing runs behind it.
 * A workspace below the query's size is MATCHA_ENOMEM, every other refusal MATCHA_EINVAL, all before any device call.  Not differentiable. */
int matcha_locus_scores(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                        const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, float* scores, float* logits,
                        int32_t lowest, int64_t* order, float* losses, void* ws, size_t ws_bytes, matcha_stream_t stream);

/* Long rows, training: matcha_forward_long_train is the chain of matcha_forward_long with every activation the backward needs kept in a
 * buffer of its own (x0, X, the LayerNorm statistics, qin / kin / vin, Q or r, O or Z -- not written over Q --, Y, H1, H2, the logits);
 * matcha_backward_long is the layer-by-layer chain of matcha_backward on that layout, with the attention backward of
 * attention_long_bwd.hip (one 32 x 32 MFMA tile per head, the probabilities recomputed from Q and K, no float atomics).  Both head
 * formulations: merged where embed_dim is a multiple of 64, the four products otherwise.  Same shapes and bounds as matcha_forward_long
 * (2 <= L <= 32; L <= 8 too, so that the pair can be held against matcha_forward / matcha_backward on identical input).
 *   opts->training, p_drop_adj / p_drop_fc1 / p_drop_pff and seed are honoured through the GEMM epilogues; the dropout counter is keyed by
 *   the token slot b L + l.  opts->status, opts->random_chrom, opts->alpha and opts->encoder_done_event as in matcha_forward /
 *   matcha_backward.  opts->deterministic, sparse_table_grad, loss_in_forward and random_chrom_dev: MATCHA_EINVAL before any device call
 *   (they belong to the L <= 8 step; the table gradient is added with float atomics as in matcha_backward without `deterministic`).
 *   logits float [B] out;  losses float [3] as matcha_forward_long, may be NULL.
 *   matcha_backward_long: dlogits float [B] (required: the loss lives with the caller), drecon float [1] or NULL, gradients ACCUMULATE
 *   into `grads`, `touched` as matcha_backward.  One backward per forward: without a matcha_forward_long_train on record for this
 *   workspace pointer it returns MATCHA_EINVAL before any launch.  The record is the one matcha_backward describes below -- one per
 *   workspace pointer for both pairs: it is consumed by the backward, dropped by a matcha_forward_long on the pointer and REPLACED by a
 *   differentiable matcha_forward there, whose record is none of matcha_backward_long's (MATCHA_EINVAL, the record stays).
 * Caller-owned memory, asynchronous on `stream`, no allocation, no host read-back.  matcha_workspace_bytes_long_train is host only and
 * returns 0 (+ matcha_last_error) for a bad argument; per token 41 d floats with merged heads, 73 d without (+ d, adj), + 8 B of
 * LayerNorm statistics and the plan's 20 B (8 B per row). */
size_t matcha_workspace_bytes_long_train(const matcha_shape* shp, int64_t B, int32_t L);
int matcha_forward_long_train(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                              const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L,
                              float* logits, float* losses, void* ws, size_t ws_bytes, matcha_stream_t stream);
int matcha_backward_long(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                         const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L,
                         const float* dlogits, const float* drecon, matcha_tensors* grads, int32_t* touched,
                         void* ws, size_t ws_bytes, matcha_stream_t stream);

/* The long rows' attention backward alone (tests): Q, dO, dQ float [T + 1, 8 d]; row_off int32 [B + 1] (row_off[B] = T: the shared padding
 * token's row).  shared_kv = 0: K, V, dK, dV float [T + 1, 8 d] per head;  shared_kv = 1 (the merged heads): K, V float [T + 1, d] that
 * every head attends, dK / dV float [T + 1, d] = the sums over the heads.  Every row of the outputs is written (dQ[T] = 0); the same call
 * gives the same bits.  No output may alias an input or another output.  2 <= L <= 32, d a multiple of 8 up to 256.
 * ws: matcha_attn_long_bwd_workspace_bytes(B, d) bytes (bounded: a fixed number of workgroups walks the hyperedges). */
size_t matcha_attn_long_bwd_workspace_bytes(int64_t B, int32_t d);
int matcha_attn_long_bwd(const float* Q, const float* K, const float* V, const float* dO, const int32_t* row_off, int64_t B, int32_t L,
                         int32_t d, int32_t shared_kv, float* dQ, float* dK, float* dV, void* ws, size_t ws_bytes, matcha_stream_t stream);

/* loss.backward() of main.py:179 for loss = bce*alpha + recon*beta, or, when `dlogits` is not NULL,
 * the vector-Jacobian product for an arbitrary upstream gradient on the logits (autograd glue).
 * Gradients are ACCUMULATED into `grads` (same layout as params; caller zeroes them -- the fused AdamW
 * does).  `touched` (device int32 [2+2C], may be NULL) receives 1 for each tensor group that received a
 * gradient this step: [0] always 1, [1] table, [2+i] adj encoder of chromosome i, [2+C+i] recon head i --
 * these are the tensors whose grad is not None in the reference (SURVEY.md §7 "AdamW semantics").
 * The call CONSUMES the activations its forward left in `ws` (gradients overwrite them): one backward per forward,
 * as loss.backward() without retain_graph.  The library keeps a host-side record per workspace pointer of the last
 * differentiable forward: it is written by a forward without opts->forward_only, dropped by a forward WITH it (which
 * keeps nothing for a backward and overwrites what was there) and dropped by the backward that consumed it.
 * matcha_forward_long_train and matcha_forward_long write and drop the SAME record, so whichever forward ran last on
 * a pointer decides which backward it takes.
 * matcha_backward on a workspace without a record of a matcha_forward -- never used, last used by a forward_only
 * forward or by one of the long rows' forwards, already consumed by a backward, or evicted (the 4096 most recent
 * workspaces are remembered) -- returns MATCHA_EINVAL before any launch. */
int matcha_backward(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                    const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L,
                    const float* y, const float* w, const float* dlogits, const float* drecon,
                    matcha_tensors* grads, int32_t* touched,
                    void* ws, size_t ws_bytes, matcha_stream_t stream);

/* The two training objectives of the reference (task_mode, main.py:532).  matcha_forward / matcha_backward are the BCE case. */
#define MATCHA_OBJECTIVE_BCE 0          /* weighted BCE on the logits (main.py:56) */
#define MATCHA_OBJECTIVE_SOFTPLUS_MSE 1 /* mse_loss(softplus(logits), y), an unweighted mean over the B rows (main.py:60-117) */

/* matcha_forward / matcha_backward with the objective chosen per call; every other argument is theirs.  Under
 * MATCHA_OBJECTIVE_SOFTPLUS_MSE `y` holds the regression targets, `w` is ignored (may be NULL), losses[0] is the MSE and
 * the logit gradient is alpha * 2 (softplus(z) - y) softplus'(z) / B (torch's softplus: z > 20 ? z : log1p(exp(z))).
 * An unknown objective returns MATCHA_EINVAL before any device call. */
int matcha_forward_objective(int32_t objective, const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                             const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L,
                             const float* y, const float* w, float* logits, float* losses,
                             void* ws, size_t ws_bytes, matcha_stream_t stream);
int matcha_backward_objective(int32_t objective, const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                              const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L,
                              const float* y, const float* w, const float* dlogits, const float* drecon,
                              matcha_tensors* grads, int32_t* touched,
                              void* ws, size_t ws_bytes, matcha_stream_t stream);

/* model.get_node_embeddings(x) (Modules.py:252-259), eval mode: rows float [T,d] for ids int64 [T].
 * `status`: optional device status word (ids outside [0, n_nodes] are flagged and read as id 0). */
int matcha_node_embeddings(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                           const int64_t* ids, int64_t T, float* rows, void* ws, size_t ws_bytes,
                           int32_t* status, matcha_stream_t stream);

/* Classifier.get_embedding(x) (Modules.py:261-276): the encoder's two outputs in the reference's padded layout,
 *   dynamic float [B,L,d] = pff_n1(...) * non_pad_mask (Modules.py:614; zero rows at padding slots)
 *   static  float [B,L,d] = tanh(next_w(node + attribute))  (:270; padding slots hold tanh(next_w(attribute_nn.bias)))
 *   attn    float [B,8,L,L], optional (may be NULL): attention probabilities in the ragged form of matcha_attn_fwd -- row i of
 *           hyperedge b and head h holds the probabilities of its k_b real keys in columns j < k_b and the probability of EACH
 *           padding slot in column k_b (all L - k_b padding keys are equal); rows i >= k_b (padding queries) are not computed
 * computed by the layer-by-layer kernels; opts as for matcha_forward (training = dropout with opts->seed).  `ws` needs
 * matcha_workspace_bytes(shp, B, L) bytes.  Not differentiable through this entry point. */
int matcha_get_embedding(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                         const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, float* dynamic,
                         float* static_, float* attn, float* losses /* [3] as matcha_forward (bce unused), may be NULL */,
                         void* ws, size_t ws_bytes, matcha_stream_t stream);

/* Row-sparse view of the table gradient of the LAST matcha_backward on `ws` that ran with opts->sparse_table_grad = 1
 * (table mode): one (node id, gradient row) pair per token of the batch, NOT yet summed per node (at 1 M nodes a batch holds
 * few repeated ids, so the per-token list is what the data-parallel exchange ships; the receiver sums, matcha_scatter_rows).
 * Pointers into `ws` (valid until the next call on it):
 *   *ids      device int32 [cap]    node id of each list entry; 0 = unused entry (skip)
 *   *rows     device float [cap,d]  gradient row of each entry (rows of unused entries hold garbage)
 *   *n_tokens device int32 [1]      number of used entries (they are the first *n_tokens[0] ones); may be passed NULL
 *   *cap      = B*L + 1 entries (the host-known bound a fixed-size all-gather is sized for). */
int matcha_table_grad_rows(const matcha_shape* shp, int64_t B, int32_t L, void* ws, size_t ws_bytes,
                           const int32_t** ids, const float** rows, const int32_t** n_tokens, int64_t* cap);

/* Sum (ids, rows) lists into a dense gradient table deterministically: the n entries (ids int32 [n], 0 = unused entry;
 * rows float [n,d]) -- e.g. the all-gathered lists of every rank, concatenated in rank order -- are stably sorted by id, the
 * rows of equal ids are added in list order, and each sum is added to dtable[id] by ONE writer (plain stores, no atomics):
 * bitwise reproducible.  Rows of ids that do not occur are not touched.  `ws`: matcha_scatter_rows_workspace_bytes bytes,
 * 256-byte aligned.  This is also the embedding backward of matcha_backward in table mode (nn.Embedding, Modules.py:29-34). */
size_t matcha_scatter_rows_workspace_bytes(int64_t n, int32_t d, int32_t n_nodes);
int matcha_scatter_rows(const int32_t* ids, const float* rows, int64_t n, int32_t d, int32_t n_nodes, float* dtable,
                        void* ws, size_t ws_bytes, matcha_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * torch.optim.AdamW(lr=1e-3) as main.py:630/:671 builds it, fused over one flat buffer.
 * Segment s covers elements [seg_off[s], seg_off[s+1]) (device int64 [n_seg+1]) and is one tensor of the
 * reference: it has its own step count `seg_step[s]` (device int32, incremented here) and is skipped
 * entirely -- no decay, no step -- unless touched[seg_group[s]] != 0 (device int32 arrays; `touched` is what
 * matcha_backward wrote; NULL = every segment is active), which is how tensors with grad None behave.
 * Gradients are zeroed after use (opt.zero_grad of main.py:175-176).  `grad_scale` multiplies the gradient
 * first (1/world_size after an all-reduce SUM).  `seg_coef` is device scratch, 3*n_seg floats.
 * ------------------------------------------------------------------------------------------ */
int matcha_adamw_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const int64_t* seg_off, int32_t n_seg, const int32_t* seg_group, const int32_t* touched,
                      int32_t* seg_step, float* seg_coef, double lr, double beta1, double beta2, double eps,
                      double weight_decay, double grad_scale, matcha_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Negative sampling (main.py:361-459) against an exact device hash set of the positive hyperedges
 * (the reference uses a Bloom filter per size, utils.py:75-97; an exact set is strictly stronger).
 * ------------------------------------------------------------------------------------------ */
/* bytes for a set holding `n_edges` hyperedges */
size_t matcha_hashset_bytes(int64_t n_edges);
/* build: edges int64 [n_edges, L] zero-padded rows (k = number of non-zero entries, ascending) */
int matcha_hashset_build(void* set, size_t set_bytes, const int64_t* edges, int64_t n_edges, int32_t L,
                         matcha_stream_t stream);
/* out[i] = 1 if row i of `rows` [n,L] is in the set */
int matcha_hashset_contains(const void* set, const int64_t* edges, int32_t L_set, const int64_t* rows,
                            int64_t n, int32_t L, int32_t* out, matcha_stream_t stream);
/* generate_negative: for each positive row (int64 [P,L], zero-padded) emit `neg_num` corrupted copies into
 * neg int64 [P*neg_num, L] (row P*? layout: negatives of positive j at rows neg_num*j .. neg_num*j+neg_num-1,
 * main.py:383-428).  node2chrom int32 [n_nodes+1]; chrom_range int32 [n_chrom,2] = [start,end) ids; an EMPTY set
 * (n_set_edges == 0) reproduces the reference's phase-1 quirk: negatives == positives (main.py:589).
 * `status` (optional device int32[4]): nodes outside [1, n_nodes] or without a chromosome are kept unchanged and flagged;
 * status[1] counts the negatives whose trials were exhausted (returned equal to the positive). */
int matcha_neg_sample(const void* set, const int64_t* set_edges, int64_t n_set_edges, int32_t L_set,
                      const int64_t* pos, int64_t P, int32_t L, int32_t neg_num, int32_t min_dis,
                      const int32_t* node2chrom, int32_t n_nodes, const int32_t* chrom_range, int32_t n_chrom,
                      const uint64_t* seed, int64_t* neg, int32_t* status, matcha_stream_t stream);
/* The same three for rows of up to MATCHA_MAX_LONG_L (32) columns: 1 <= L <= 32 and 1 <= L_set <= 32, every other check as above.
 * ONE table format: a row's hash runs over its non-zero prefix and does not depend on the container's width, so a table built by
 * either build entry is read by either contains / sample entry whose width bound is met (a stored row of k <= 8 nodes in a width-25
 * set is found by a width-5 query).  matcha_hashset_bytes serves both.  matcha_neg_sample_long runs neg_sample_long_kernel: 32
 * adjacent lanes per negative, lane i = position i.  Random stream: the key, the hi counter (the negative's index) and the mask
 * counters of matcha_neg_sample; the replacement counter is S*trial + position with S = 8 when L <= 8 -- bit for bit
 * matcha_neg_sample's negatives -- and S = 32 when L > 8.  P * neg_num < 2^31. */
int matcha_hashset_build_long(void* set, size_t set_bytes, const int64_t* edges, int64_t n_edges, int32_t L,
                              matcha_stream_t stream);
int matcha_hashset_contains_long(const void* set, const int64_t* edges, int32_t L_set, const int64_t* rows,
                                 int64_t n, int32_t L, int32_t* out, matcha_stream_t stream);
int matcha_neg_sample_long(const void* set, const int64_t* set_edges, int64_t n_set_edges, int32_t L_set,
                           const int64_t* pos, int64_t P, int32_t L, int32_t neg_num, int32_t min_dis,
                           const int32_t* node2chrom, int32_t n_nodes, const int32_t* chrom_range, int32_t n_chrom,
                           const uint64_t* seed, int64_t* neg, int32_t* status, matcha_stream_t stream);

/* Planted outliers (the reference's generate_outlier_part, History_version/Code/utils.py:184-233): `draws` copies of every positive
 * (int64 [P,L] zero-padded ascending, 1 <= L <= 32) with ONE locus replaced by a foreign bin of the same chromosome.  Local row i is global
 * row n = n0 + i, a copy of positive i / draws (n0 >= 0; a caller that cuts its positives into chunks passes n0 = draws * (positives in front
 * of the chunk), so that n / draws is the positive and n % draws the copy, and gets the rows of one call).  k = the positive's non-zero prefix.  Counter RNG of oracle/rng.py,
 * stream 18, hi counter n:
 *   position   p = (n % draws) % k with `cycle`, else (rand(key, n, 0xFFFF0000) * k) >> 32;
 *   trial t    (0 .. 255) bin j = start + ((rand(key, n, t) * (end - start)) >> 32) in the chromosome of the positive's locus p; cand = the
 *              positive without locus p plus j, ascending.  Refused: j is a locus of the positive; an adjacent gap of cand <= min_dis;
 *              (pair set given) a pair (min(j, v), max(j, v)), v another locus of cand, is in the pair set; (set given) cand is in the set.
 *   out        int64 [P*draws, L] = cand zero-padded; planted int32 [P*draws] = the index of j in cand.
 * No plant -- 256 trials exhausted, k < 2, a locus outside [1, n_nodes], locus p without a chromosome: the row is a copy of the positive and
 * planted = -1.  status (optional device int32[4]): [0] |= MATCHA_STATUS_BAD_CHROM for the last two, [1] += rows whose trials were exhausted.
 * Both sets are tables of matcha_hashset_build(_long) over their edge lists; n_*_edges == 0 switches that refusal off (buffers may be NULL).
 * Every argument check of matcha_neg_sample_long; P*draws and n0 + P*draws below 2^31.  outlier_plant_kernel: 32 lanes per row. */
int matcha_outlier_plant(const void* set, const int64_t* set_edges, int64_t n_set_edges, int32_t L_set,
                         const void* pair_set, const int64_t* pair_edges, int64_t n_pair_edges, int32_t L_pair,
                         const int64_t* pos, int64_t P, int32_t L, int32_t draws, int32_t cycle, int32_t min_dis,
                         const int32_t* node2chrom, int32_t n_nodes, const int32_t* chrom_range, int32_t n_chrom,
                         const uint64_t* seed, int64_t n0, int64_t* out, int32_t* planted, int32_t* status, matcha_stream_t stream);

/* Biased second-order random walks over the hypergraph (the reference's History_version/Code/random_walk_hyper.py): walks
 * w0 <= w < w1, walk w starting at nodes[w % n_start], out int32 [(w1 - w0), walk_length] (row w - w0), node ids 0 .. n_nodes.
 * Tables (matcha_amd/walk.py builds them): inc_ptr int64 [n_nodes + 2], and per incidence (edge e of node v, c another node of e) the
 * neighbour inc_nb and inc_cum, the inclusive prefix WITHIN the node of the integer weight max(1, rint(2^40 deg(c)^-1/2 / |e|)); the
 * pair and the triple set are tables of matcha_hashset_build over all 2- and 3-subsets of the hyperedges (n_*_edges == 0: no such
 * subset, buffers may be NULL); thresholds is a HOST int64[3] for the classes back (1/p), pair (1) and far (1/q): floor(2^32 alpha /
 * alpha_max), 2^32 = accepts always.  Counter RNG of oracle/rng.py, stream 19, hi = w, lo = step << 18 | trial << 2 | draw.  Step s >= 1
 * from dst (previous node src):
 *   proposal   c = inc_nb[first i with inc_cum[i] > mulhi64(rand64(draws 0, 1), the node's total)];  step 1 takes it;
 *   class      back if c == src or {src, dst, c} is in the triple set, else pair if {src, c} is in the pair set, else far;
 *   accepted   when rand(draw 2) < thresholds[class]; otherwise the next trial, at most max_trials (1 .. 65536): then the last
 *              proposal stands and status[1] += 1 (status: optional device int32[4]).
 * A node without incidences repeats itself.  A start outside 0 .. n_nodes gives an all-zero row and status[0] |= MATCHA_STATUS_BAD_ID.
 * walk_length 1 .. 16384, 0 <= w0, w1 < 2^31.  hyper_walk_kernel: one lane per walk. */
int matcha_hyper_walk(const int64_t* inc_ptr, const int32_t* inc_nb, const uint64_t* inc_cum, int32_t n_nodes,
                      const void* pair_set, const int64_t* pair_edges, int64_t n_pair_edges, int32_t L_pair,
                      const void* triple_set, const int64_t* triple_edges, int64_t n_triple_edges, int32_t L_triple,
                      const int64_t* thresholds, const int32_t* nodes, int64_t n_start, int64_t w0, int64_t w1,
                      int32_t walk_length, int32_t max_trials, const uint64_t* seed, int32_t* out, int32_t* status,
                      matcha_stream_t stream);

/* One pass of skip-gram with negative sampling (word2vec) over walks w0 <= w < w1 of walks int32 [n_walks, walk_length] (ids 1 .. n_nodes):
 * syn0 / syn1 float [n_nodes + 1, d], d = 64, 128 or 256, updated in place with float atomics -- NOT bitwise reproducible from run to run.
 * noise_cum uint64 [n_nodes + 1]: the inclusive prefix of the nodes' integer noise weights, entry 0 (no node) = 0.  The global position of
 * (w, i) is g = g_base + w walk_length + i (g_base = epoch * n_walks * walk_length) of g_total <= 2^32 positions in all; the rule per
 * position is stated at the top of csrc/sgns.hip (stream 20, hi = g).  window 1 .. 1024, negative 0 .. 32, lr0 >= lr1 >= 0.  An id outside
 * 1 .. n_nodes trains nothing and sets status[0] |= MATCHA_STATUS_BAD_ID (status: optional device int32[4]).  sgns_kernel: one wavefront
 * per position. */
int matcha_sgns_epoch(const int32_t* walks, int64_t n_walks, int32_t walk_length, int64_t w0, int64_t w1, int32_t n_nodes,
                      int32_t d, float* syn0, float* syn1, const uint64_t* noise_cum, int32_t window, int32_t negative,
                      double lr0, double lr1, int64_t g_base, int64_t g_total, const uint64_t* seed, int32_t* status,
                      matcha_stream_t stream);

/* The bookkeeping of one step of the reference's epoch loop (main.py:155-188) on the device, so that an epoch can replay one captured
 * step (matcha_amd/train.py).  `it` is a device int64 step counter.
 * matcha_step_select (main.py:160-161, Modules.py:192): x[0:P] = pos[it*P .. it*P+P) (rows of the epoch's shuffled positives,
 * int64 [n_rows, L]; indices wrap around modulo n_rows), ww[0:P] = w[it*P ..], and, when `cell` is given, cell[0] = chroms[it] (the step's reconstruction chromosome);
 * seed0 / seed1 (optional device uint64): counter-RNG seeds to advance by one (the sampler's and the dropout masks').
 * matcha_step_record (main.py:58, :185-188, :449-451): preds[it][b] = sigmoid(logits[b]), sizes[it][b] = non-zero entries of x[b]
 * (x int64 [B, L]), sums[0] += losses[0] (bce), sums[1] += losses[1] (recon), then it += 1.  preds / sizes are [n_steps, B]. */
int matcha_step_select(const int64_t* pos, const float* w, int64_t n_rows, int32_t L, const int64_t* it, int32_t P, int64_t* x,
                       float* ww, const int32_t* chroms, int64_t n_chroms, int32_t* cell, uint64_t* seed0, uint64_t* seed1,
                       matcha_stream_t stream);
int matcha_step_record(const float* logits, const float* losses, const int64_t* x, int64_t B, int32_t L, int64_t* it, int64_t n_steps,
                       float* sums, float* preds, int64_t* sizes, matcha_stream_t stream);
/* matcha_step_record_pairs: the regression counterpart of matcha_step_record (main.py:60-117): same counter, same loss sums, same
 * past-the-end guard.  The B rows are paired by a bijection pi of [0, B) drawn from (seed[0], it) -- a 6-round Feistel network
 * over the next even power of two with cycle walking (tests/test_cpu_regress.py restates it) -- and for every pair
 * j < B/2 of rows r0 = pi(2j), r1 = pi(2j+1), with y the targets float [B]:
 *   preds[it][j]  = sigmoid(softplus(logits[r0]) - softplus(logits[r1]))
 *   labels[it][j] = y[r0] == y[r1] ? -1 (masked pair) : (y[r1] < y[r0] ? 1 : 0)      (torch.argmin of the pair)
 *   sizes[it][j]  = non-zero entries of x[r0]
 * preds / labels / sizes are [n_steps, B/2]. */
int matcha_step_record_pairs(const float* logits, const float* losses, const float* y, const int64_t* x, int64_t B, int32_t L,
                             int64_t* it, int64_t n_steps, const uint64_t* seed, float* sums, float* preds, int32_t* labels,
                             int64_t* sizes, matcha_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Op-level entry points (the kernels behind matcha_forward/backward, exposed so that each one is
 * parity-tested on its own against the oracle).
 * ------------------------------------------------------------------------------------------ */
#define MATCHA_GEMM_NT 0 /* C[M,N] = A[M,K] . B[N,K]^T   (F.linear, Modules.py:111/:392/:481-483/:340)   */
#define MATCHA_GEMM_NN 1 /* C[M,N] = A[M,K] . B[K,N]     (input gradient of a Linear)                     */
#define MATCHA_GEMM_TN 2 /* C[M,N] = A[R,M]^T . B[R,N]   (weight gradient; reduction over R rows/tokens)  */

/* epilogue steps, applied in THIS order: */
#define MATCHA_EPI_BIAS 1        /* + bias[n]                                                         */
#define MATCHA_EPI_TANH 2        /* tanh()                                                            */
#define MATCHA_EPI_RESIDUAL 16   /* + residual[m,n]                                                   */
#define MATCHA_EPI_DROPOUT 4     /* * keep/(1-p); keep = rand_u32(key(seed,stream), m, n) >= p*2^32   */
#define MATCHA_EPI_ROWMASK 8     /* * (row_ids[m] != 0)                                               */
#define MATCHA_EPI_DTANH 32      /* * (1 - (aux[m,n]*aux_scale)^2)   aux = saved tanh output          */
#define MATCHA_EPI_ACCUM 64      /* C += result instead of C = result                                 */

typedef struct matcha_gemm_epilogue {
  int32_t flags;
  const float* bias;        /* [N] */
  const float* residual;    /* [M,N] */
  const float* aux;         /* [M,N] */
  const int64_t* row_ids;   /* [M] node ids (row mask) */
  const uint64_t* seed;     /* device */
  int32_t stream_id;        /* RNG stream (oracle/rng.py) */
  float p_drop;
  float aux_scale;          /* (1-p) when aux holds dropout(tanh(.)), else 1 */
} matcha_gemm_epilogue;

/* f32 MFMA GEMM. For TN, `ws` must hold matcha_gemm_tn_workspace_bytes(M,N,R) bytes; `colsum` (may be
 * NULL) additionally receives sum_r A[r,m] (bias gradient), accumulated like C.
 * The contraction length (K; R for TN) must be >= 1 and M, N >= 0: anything else is MATCHA_EINVAL before any launch
 * (an empty sum has no defined epilogue here).  M == 0 or N == 0 is a no-op that returns MATCHA_OK. */
size_t matcha_gemm_tn_workspace_bytes(int64_t M, int64_t N, int64_t R);
int matcha_gemm(int32_t op, const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K,
                const matcha_gemm_epilogue* epi, float* colsum, const int64_t* b_row_gather,
                void* ws, size_t ws_bytes, matcha_stream_t stream);

/* The ragged execution plan of a batch (csrc/ragged.hip): the real slots (x != 0, get_non_pad_mask Modules.py:12-14) of the
 * zero-padded x [B,L] (pad_sequence, main.py:435-437) compacted into a CSR token list + ONE shared padding token, and tiles of
 * whole hyperedges (<= 63 tokens) for the fused kernels.  matcha_forward builds it inside its workspace; this entry point
 * builds it alone so that it can be compared bit for bit with the C restatement oracle/c/ragged_plan.c.
 *   view->row_off  int32 [B+1]; tok_slot, tok_key, tok_pos int32 [B*L+1]; tok_id int64 [B*L+1]; count int32 [4] = {Tr+1, Tr,
 *   tiles, half tiles}; tile_meta int32 [tiles_cap][4] = {first token, tokens, first hyperedge, hyperedges}; half_meta: the same
 *   stream cut into half tiles of <= 31 tokens (one wavefront each in the fused forward) -- device pointers into `ws`. */
typedef struct matcha_ragged_view {
  const int32_t* row_off; const int32_t* tok_slot; const int64_t* tok_id; const int32_t* tok_key; const int32_t* tok_pos;
  const int32_t* count; const int32_t* tile_meta; int64_t tiles_cap;
  const int32_t* half_meta; int64_t halves_cap;   /* half tiles: whole hyperedges, <= 31 tokens, same four fields; count[3] of them */
  const int32_t* tok_tile;                        /* int32 [B*L+1]: (tile << 6) | row of each token inside tile_meta's tiling        */
} matcha_ragged_view;
size_t matcha_ragged_plan_bytes(int64_t B, int32_t L);
int matcha_ragged_plan(const int64_t* x, int64_t B, int32_t L, int32_t n_nodes, int32_t* status, void* ws, size_t ws_bytes,
                       matcha_ragged_view* view, matcha_stream_t stream);

/* K1 + K6: x0[t] = rows[t] + attr_table[x[t]] . attr_w^T + attr_b, rows[t] = table[x[t]] (table != NULL) or
 * dense[t] (Modules.py:34, :263-269).  Backward: scatter-add into dtable (row 0 skipped, padding_idx=0). */
int matcha_embed_fwd(const int64_t* x, int64_t T, int32_t d, const float* table, const float* dense,
                     const float* attr_table, int32_t n_attr, const float* attr_w, const float* attr_b,
                     float* x0, matcha_stream_t stream);
int matcha_embed_scatter_bwd(const int64_t* x, int64_t T, int32_t d, const float* dx0, float* dtable,
                             matcha_stream_t stream);

/* K8 (LayerNorm part): xhat-normalise X once, emit the three affine variants (Modules.py:519-521). */
int matcha_ln3_fwd(const float* X, int64_t T, int32_t d, const float* gq, const float* bq, const float* gk,
                   const float* bk, const float* gv, const float* bv, float* qin, float* kin, float* vin,
                   float* stats /* [T,2] mean,rstd */, matcha_stream_t stream);

/* K9: per (hyperedge, head) attention with the diagonal masked and pad slots attended (Modules.py:449-458;
 * SURVEY.md headline fact 7), on the ragged token layout: hyperedge b owns the compact token rows
 * [row_off[b], row_off[b+1]) (k_b = their number <= L real nodes), row row_off[B] is the ONE shared padding token
 * whose K/V stand for each of the L - k_b padding slots of the batch-wide [B, L] layout.
 * Q,K,V,O,dQ,dK,dV: [row_off[B] + 1, 8d]; P: [B, 8, L, L] (row i: real columns j < k_b, then the per-slot
 * padding probability in column k_b).  row_off: device int32 [B+1].  bwd also writes dK/dV (and dQ = 0) of the
 * padding token row; `ws` needs matcha_attn_bwd_workspace_bytes(B, d) bytes. */
size_t matcha_attn_bwd_workspace_bytes(int64_t B, int32_t d);
int matcha_attn_fwd(const float* Q, const float* K, const float* V, const int32_t* row_off, int64_t B, int32_t L,
                    int32_t d, float* O, float* P, matcha_stream_t stream);
int matcha_attn_bwd(const float* Q, const float* K, const float* V, const float* P, const float* dO,
                    const int32_t* row_off, int64_t B, int32_t L, int32_t d, float* dQ, float* dK, float* dV,
                    void* ws, size_t ws_bytes, matcha_stream_t stream);

/* ---- k-mer generation (Code/generate_kmers.py:8-69, one k-mer size per call) -------------------------
 * Every ascending k-subset of a cluster whose adjacent node gaps all exceed `min_dis` (generate_kmers.py:17, :24-32),
 * counted over all clusters (:34-37), kept when seen >= `min_freq` times (:40).
 *   ids, offsets   clusters in CSR form: cluster c = ids[offsets[c] .. offsets[c+1]), sorted unique node ids
 *                  (process.py:66-77), device int32 / int64 [n_clusters + 1]
 *   comb_off       device int64 [n_clusters + 1]: exclusive prefix sums of C(len_c, k) over the clusters with
 *                  k <= len_c <= max_cluster_size (<= 64; generate_kmers.py:88) and 0 for the others -- the caller has the
 *                  cluster lengths on the host; total_combos = comb_off[n_clusters] < 2^32 - 1
 *   out_kmers      int64 [cap, k] rows in lexicographic order (the reference's order depends on worker scheduling),
 *   out_freq       int64 [cap], n_out: device int64, the number of k-mers kept (if > cap only the first cap are written)
 *   ws             matcha_kmer_workspace_bytes(total_combos, k, n_nodes) bytes */
size_t matcha_kmer_workspace_bytes(int64_t total_combos, int32_t k, int32_t n_nodes);
int matcha_kmer_generate(const int32_t* ids, const int64_t* offsets, const int64_t* comb_off, int64_t n_clusters,
                         int64_t total_combos, int32_t k, int32_t n_nodes, int32_t min_dis, int32_t min_freq,
                         int64_t* out_kmers, int64_t* out_freq, int64_t cap, int64_t* n_out, void* ws, size_t ws_bytes,
                         matcha_stream_t stream);

/* ---- positive-weight preprocessing (Code/main.py:555, :653) -------------------------------------------
 * The uniform quantile transform of one float32 column of k-mer frequencies: what
 * sklearn.preprocessing.QuantileTransformer(n_quantiles, output_distribution='uniform').fit_transform computes when it fits
 * on every row (subsample=None; above 10 000 rows scikit-learn's default fits on a random subsample -- the reference's only
 * non-determinism here, deliberately not reproduced).  Bit-identical to oracle/positives.py.
 *   freq           device float32 [n], 1 <= n < 2^31, no NaNs (frequencies are counts)
 *   n_quantiles    1 .. 4096 (the reference uses 1000); clamped to n as scikit-learn does
 *   out            device float32 [n] in [0, 1]; must not alias freq
 *   quantiles_out  optional device float64 [min(n_quantiles, n)]: the fitted landmarks (QuantileTransformer.quantiles_)
 *   ws             matcha_quantile_workspace_bytes(n) bytes */
size_t matcha_quantile_workspace_bytes(int64_t n);
int matcha_quantile_uniform(const float* freq, int64_t n, int32_t n_quantiles, float* out, double* quantiles_out, void* ws,
                            size_t ws_bytes, matcha_stream_t stream);

/* ---- feature construction from contact maps ----------------------------------------------------------
 * matcha_pixels_to_adj   Code/process.py:144-172: cooler pixels -> adjacency.  For every pixel i whose two bins map to nodes
 *   (index2node[bin] >= 1; 0 = chromosome outside chrom_list) and whose count is not NaN: M[n1-1][n2-1] += count and
 *   M[n2-1][n1-1] += count, M = intra when node2chrom[n1] == node2chrom[n2], else inter.  Adds into the caller's matrices
 *   (zero them first; call repeatedly to stream a large pixel table).
 *     bin1, bin2 device int64 [n_pixels]; count device float64 [n_pixels]; index2node device int32 [n_index];
 *     node2chrom device int32 [n_nodes + 1] (entry 0 unused); intra, inter device float64 [n_nodes, n_nodes]
 * matcha_corrcoef_block  Code/main.py:571-575: np.corrcoef of one chromosome's intra block, NaN -> 0.
 *     adj device float32, the block's top-left element, row stride ld (elements); out device float32 [n, n];
 *     ws matcha_corrcoef_workspace_bytes(n) bytes.  float64 arithmetic; differs from numpy only by summation order.
 * matcha_zscore_rows     Code/Modules.py:146-152: every row of a float32 [rows, cols] matrix, in place: strictly positive
 *     entries -> (x - mean) / std (ddof 0) over those entries, then NaN -> 0. */
int matcha_pixels_to_adj(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t n_pixels,
                         const int32_t* index2node, int64_t n_index, const int32_t* node2chrom, int32_t n_nodes,
                         double* intra, double* inter, matcha_stream_t stream);
size_t matcha_corrcoef_workspace_bytes(int32_t n);
int matcha_corrcoef_block(const float* adj, int64_t ld, int32_t n, float* out, void* ws, size_t ws_bytes,
                          matcha_stream_t stream);
int matcha_zscore_rows(float* matrix, int64_t rows, int64_t cols, matcha_stream_t stream);

/* ---- contact matrices from the clusters (Code/process.py:90-105 edgelist2adj; History_version/Code/main_drop.py:543-563 get_adjacency;
 * DESIGN.md 7.18; csrc/cluster_adj.hip) --------------------------------------------------------------------------------------------
 * Clusters as CSR: ids device int32 [I], node ids 1 .. n_nodes strictly ascending inside a cluster; offsets int64 [M + 1] with
 * offsets[M] = I; a cluster holds 2 .. 65535 nodes (clusters of 0 or 1 nodes have no pairs and are passed over).
 * matcha_cluster_pairs_count   host only: the sum over the clusters of s (s - 1) / 2 from a HOST copy of offsets; -1 when a cluster has more
 *     than 65535 nodes (or a negative length), the sum leaves int63, or an argument is invalid.
 * matcha_cluster_adj_update    q device int64 [M]: the clusters' weights in fixed point, rint(w 2^32); pair_ptr device int64 [M + 1]: pair_ptr[0]
 *     = 0, pair_ptr[c + 1] = pair_ptr[c] + s_c (s_c - 1) / 2 (made on the host).  Every pair i < j of every cluster adds q[c] to
 *     acc[(id_i - 1) n_nodes + (id_j - 1)] with one 64-bit integer atomic: acc, device int64 [n_nodes, n_nodes], is caller-owned, zeroed by the
 *     caller before the first call and carried from call to call; only its upper triangle is written.  The result does not depend on the order
 *     of the adds, of the clusters or on how the clusters are cut into calls.  The caller keeps the sum of |q| below 2^62 (a cell receives at
 *     most one add per cluster).  A cluster whose ids are not strictly ascending or leave 1 .. n_nodes, or whose offsets disagree with
 *     pair_ptr, adds nothing and sets status[0] |= MATCHA_STATUS_BAD_ID (status: optional device int32[4]).  M = 0 launches nothing.
 *     cluster_pairs_update_kernel: 2048 blocks, every wavefront one contiguous run of global pair ranks.
 * matcha_cluster_adj_finish    acc -> float64 matrices, value double(acc) 2^-32 in the cell and in its mirror, diagonal 0: with inter_or_null the
 *     cell goes to intra when node2chrom[id_i] == node2chrom[id_j] (device int32 [n_nodes + 1], entry 0 unused) and to inter otherwise, the
 *     other matrix's cell is written 0; without it everything goes to intra (edgelist2adj's matrix; node2chrom may be NULL).  Overwrites every
 *     element of its outputs; acc is left as it is.  cluster_adj_finish_kernel.
 * matcha_block_colmax_normalise   get_adjacency(norm=True): for every range k, rows [ranges[2 k], ranges[2 k + 1]) (device int64 [n_ranges, 2],
 *     0-based, clipped to [0, n_nodes); the ranges must not overlap) and every column: A[rows, col] /= max(A[rows, col]) + 1e-10, float64, in
 *     place on A [n_nodes, n_nodes].  ws (matcha_block_colmax_workspace_bytes, 8-byte aligned) keeps the maxima as float64 [n_ranges, n_nodes].
 *     n_ranges = 0 launches nothing.  block_colmax_normalise_kernel.
 * Every refusal (a null pointer, n_nodes < 1, M or n_ranges out of range, a workspace that is too small) is MATCHA_EINVAL with a message,
 * before any device call. */
int64_t matcha_cluster_pairs_count(const int64_t* offsets_host, int64_t M);
int matcha_cluster_adj_update(const int32_t* ids, const int64_t* offsets, const int64_t* q, const int64_t* pair_ptr, int64_t M,
                              int32_t n_nodes, int64_t* acc, int32_t* status, matcha_stream_t stream);
int matcha_cluster_adj_finish(const int64_t* acc, const int32_t* node2chrom, int32_t n_nodes, double* intra, double* inter_or_null,
                              matcha_stream_t stream);
size_t matcha_block_colmax_workspace_bytes(int32_t n_nodes, int32_t n_ranges);
int matcha_block_colmax_normalise(double* A, int32_t n_nodes, const int64_t* ranges, int32_t n_ranges, void* ws, size_t ws_bytes,
                                  matcha_stream_t stream);

/* ---- the cluster file's text -> clusters in CSR form (Code/process.py:42-87 parse_file; csrc/cluster_text.hip) -----------
 * One chunk of WHOLE lines of a SPRITE-style cluster file (id <tab> chr:pos <tab> ...), as bytes on the device, becomes the CSR that
 * matcha_kmer_generate and matcha_cluster_adj_update take: ids device int32, offsets device int64.  Integer work: for every text it accepts
 * the result is the reference's parse_file bit for bit.
 *   lines      every '\r' and every '\n' ends a line; a last line without a terminator counts
 *   strip      leading / trailing bytes 0x09-0x0d, 0x1c-0x1f, 0x20 are removed, the rest is split on '\t', the first field (the id) is dropped
 *   pre-filter a line of fewer than 2 or more than 50 max_cluster_size items is skipped unparsed: nothing on it is an error
 *   items      exactly one ':' (else _ESPLIT); an item whose name is not in the table is dropped before its position is read; node id =
 *              first_node + floor(position / res); a bin >= n_bins is _EBIN
 *   cluster    ids de-duplicated and ascending; kept when 2 <= ids <= max_cluster_size; kept clusters stay in file order
 * NARROWER than Python's int(): a position is 1 .. 18 ASCII digits.  "+5", " 5", "2_500", "-5", "x" and the empty string are _EGRAMMAR (the
 * host parser takes the first three and answers KeyError to the fourth); 19 or more digits are _EBIN; a byte >= 0x80 anywhere in the text,
 * skipped lines included, is _ENONASCII (Python's strip would also strip some non-ASCII blanks).
 * The chromosome table (HOST arrays, checked and copied by the call): names char [n_chrom][MATCHA_CLUSTER_TEXT_NAME_MAX], each 1 .. 32 bytes
 * above 0x20 and below 0x80 without ':', zero-padded, no two alike, compared exactly ("chr1", "chr10" and "chr1_random" are three names);
 * at most MATCHA_CLUSTER_TEXT_CHROM_MAX = 256 of them; first_node / n_bins int32 [n_chrom] with 1 <= first_node and first_node + n_bins - 1 <=
 * n_nodes and n_bins * res <= 2^53 (build_node_dict: n_bins = ceil(size / res) + 1).
 * matcha_cluster_text_count   counts device int64 [2] <- {lines, tabs} of text (device uint8 [n], 16-byte aligned, n < 2^31); lines = terminators
 *     + 1.  The caller reads them (one host sync per chunk) and sizes the workspace and the outputs from them.
 * matcha_cluster_text_parse   n_lines / n_tabs as counted (the kernels check them against the text: a mismatch writes nothing and sets _ECOUNT);
 *     ids [ids_cap >= n_tabs], offsets [offsets_cap >= n_lines + 1]; n_clusters, n_ids device int64 [1]; offsets[0 .. n_clusters] and
 *     ids[0 .. n_ids) are written.  status device int32 [8], OVERWRITTEN: [0] the MATCHA_CLUSTER_TEXT_E* bits, [1] / [2] / [3] the least byte
 *     offset of an item that is _ESPLIT / _EBIN / _EGRAMMAR, [4] the least offset of a byte >= 0x80 (INT32_MAX where there is none).  With an
 *     error bit set the CSR is not to be used.  ws: matcha_cluster_text_workspace_bytes(n, n_lines, n_tabs) bytes, 256-byte aligned.
 * Every refusal (a size out of range, a null or misaligned pointer, a bad table, a workspace that is too small) is MATCHA_EINVAL with a
 * message, before any device call. */
#define MATCHA_CLUSTER_TEXT_NAME_MAX 32
#define MATCHA_CLUSTER_TEXT_CHROM_MAX 256
#define MATCHA_CLUSTER_TEXT_ESPLIT 1    /* an item without exactly one ':' (the host parser's EOFError) */
#define MATCHA_CLUSTER_TEXT_EBIN 2      /* a bin past its chromosome's last (KeyError) */
#define MATCHA_CLUSTER_TEXT_EGRAMMAR 4  /* a position that is not 1 .. 18 ASCII digits (ValueError) */
#define MATCHA_CLUSTER_TEXT_ENONASCII 8 /* a byte >= 0x80 (ValueError) */
#define MATCHA_CLUSTER_TEXT_ECOUNT 16   /* n_lines / n_tabs are not the text's counts */
size_t matcha_cluster_text_count_workspace_bytes(int64_t n);
int matcha_cluster_text_count(const uint8_t* text, int64_t n, int64_t* counts, void* ws, size_t ws_bytes, matcha_stream_t stream);
size_t matcha_cluster_text_workspace_bytes(int64_t n, int64_t n_lines, int64_t n_tabs);
int matcha_cluster_text_parse(const uint8_t* text, int64_t n, int64_t n_lines, int64_t n_tabs, const char* names, const int32_t* first_node,
                              const int32_t* n_bins, int32_t n_chrom, int64_t res, int64_t max_cluster_size, int32_t n_nodes, int32_t* ids,
                              int64_t ids_cap, int64_t* offsets, int64_t offsets_cap, int64_t* n_clusters, int64_t* n_ids, int32_t* status,
                              void* ws, size_t ws_bytes, matcha_stream_t stream);

/* ---- denoised contact maps (Code/denoise_contact.py:147-207) ----------------------------------------------------------
 * One chromosome [lo, hi) of chrom_range, n = hi - lo bins, pairs (i, j) with i + min_dis <= j in generate_pair_wise order: row
 * r = i - lo holds max(0, n - min_dis - r) pairs, stored contiguously.  Bit for bit with the reference's numpy for the same inputs.
 * matcha_denoise_intra   the post-processing up to the quantile transforms (:160-188):
 *     proba        device float32 [n_pairs]: the sweep's probabilities (n_pairs = K (K + 1) / 2, K = n - min_dis)
 *     origin       device float32, element (lo - 1, lo - 1) of intra_adj, row stride origin_ld >= n (elements)
 *     my, origin_part, my_proba   device float32 [n, n]: the three matrices the reference hands to its QuantileTransformer,
 *                  my and my_proba with the gap rows / columns zeroed; none may alias another or an input
 *     gap          device uint8 [2 n]: gap1 (row sums of the observed matrix == 0) then gap2 (column sums == 0)
 *     ws           matcha_denoise_workspace_bytes(n) bytes: six coverage vectors, 24 n bytes rounded up to 256 (597 760 bytes at
 *                  n = 24 900; the matrices themselves live in the caller's outputs)
 *   Refuses, before any device call: a null pointer, n < 1 or n * n >= 2^31 (the quantile transform's limit), min_dis outside
 *   [0, n) (no pairs), an n_pairs that does not match n and min_dis, origin_ld < n, a workspace that is too small.
 * matcha_denoise_pixels  balanced = m[i - lo, j - lo] for every pair, in pair order (:205-207): out device float32 [n_pairs].
 * Deliberate differences from the reference: (a) the quantile transforms between the two calls fit on all n^2 values
 * (subsample=None; identical to scikit-learn's default up to n = 100); (b) a chromosome without pairs is refused here and skipped by
 * matcha_amd/denoise.py, where the reference crashes; (c) the .mcool container is written only when h5py imports (always an .npz). */
size_t matcha_denoise_workspace_bytes(int32_t n);
int matcha_denoise_intra(const float* proba, int64_t n_pairs, int32_t n, int32_t min_dis, const float* origin, int64_t origin_ld,
                         float* my, float* origin_part, float* my_proba, uint8_t* gap, void* ws, size_t ws_bytes,
                         matcha_stream_t stream);
int matcha_denoise_pixels(const float* m, int32_t n, int32_t min_dis, float* out, matcha_stream_t stream);

/* ---- de novo k-way sweep -------------------------------------------------------------------------------
 * Candidates of size k in the region [lo, lo + n) of node ids: strictly ascending k-tuples whose adjacent differences are all
 * >= min_gap (min_gap = min_distance + 1 is the rule of Code/generate_kmers.py:18, :33 and of the negative sampler), in
 * lexicographic order; the rank of a candidate is its position in that order, from 0.  With m = n - (k - 1)(min_gap - 1) there are
 * C(m, k) of them (0 when m < k).  Supported: 2 <= k <= 8, n >= 1, min_gap >= 1, C(m, k) < 2^63 -- a larger count is refused.
 * matcha_kway_count   host only: C(m, k), or -1 for invalid arguments or a count >= 2^63.
 * matcha_kway_rows    writes x, device int64 [count, L] with k <= L <= 8, columns k .. L-1 zero: row i is the candidate of rank
 *     rank0 + i (ranks == NULL; the range must lie inside [0, C(m, k)), else refused) or of rank ranks[i] (device int64 [count];
 *     a rank outside [0, C(m, k)) gives an all-zero row).  64-bit integer unranking, k steps per row; count = 0 launches nothing.
 *
 * Streaming selection of the best K (score, rank) pairs.  Total order: higher score first (IEEE comparison, so -0.0 == +0.0 and
 * the rank decides; +inf is the highest score, -inf the lowest), then lower rank.  A NaN score or a row with skip[i] != 0 is never
 * kept.  After any sequence of updates the state holds the best min(K, valid rows seen) pairs, and the same pairs bit for bit
 * however the rows were cut into updates (no atomics: nothing depends on arrival order).
 * matcha_topk_bytes   bytes of one state for K pairs and updates of at most max_chunk rows (1 <= K, max_chunk < 2^31); 0 when out
 *     of range.  Sized without asking the device.  K and max_chunk are passed again to the other three calls: the library keeps
 *     nothing on the host between calls and never reads the state back.
 * matcha_topk_init    empties the state (a kernel, no memset).
 * matcha_topk_update  scores device float32 [n], row i has rank rank0 + i; skip optional device int32 [n] (the layout
 *     matcha_hashset_contains writes); 0 <= n <= max_chunk, n = 0 is a no-op that launches nothing.
 * matcha_topk_read    scores_out device float32 [K], ranks_out device int64 [K], sorted in the order above; n_out device int64:
 *     the number of valid pairs (entries beyond it are score 0, rank -1).
 * All refuse, before any device call: a null pointer, K or max_chunk out of range, a state smaller than matcha_topk_bytes. */
int64_t matcha_kway_count(int32_t n, int32_t k, int32_t min_gap);
int matcha_kway_rows(int64_t lo, int32_t n, int32_t k, int32_t min_gap, int64_t rank0, const int64_t* ranks, int64_t count,
                     int32_t L, int64_t* x, matcha_stream_t stream);
size_t matcha_topk_bytes(int32_t K, int64_t max_chunk);
int matcha_topk_init(void* state, size_t bytes, int32_t K, int64_t max_chunk, matcha_stream_t stream);
int matcha_topk_update(void* state, size_t bytes, int32_t K, int64_t max_chunk, const float* scores, const int32_t* skip,
                       int64_t n, int64_t rank0, matcha_stream_t stream);
int matcha_topk_read(const void* state, size_t bytes, int32_t K, int64_t max_chunk, float* scores_out, int64_t* ranks_out,
                     int64_t* n_out, matcha_stream_t stream);

/* ---- anchored k-way sweep ------------------------------------------------------------------------------
 * The best K completions of every anchor.  An anchor row is s fixed node ids (1 <= s <= k - 1); the free part is a candidate of
 * size f = k - s of the partner region [lo, lo + n) under the rule above (f = 1: every node, C_f = n; otherwise
 * C_f = C(n - (f - 1)(min_gap - 1), f)), ranked lexicographically from 0.  With A anchor rows the global rank is g = a C_f + r
 * (anchor index a, free rank r), 0 <= g < A C_f < 2^63.  The candidate is the k ids sorted ascending (duplicates kept), zero-padded
 * to L; it is valid iff every adjacent difference is >= min_gap.  Invalid candidates keep their rank and their row; a flag marks them.
 * matcha_kway_anchor_count  host only: A C_f, or -1 for invalid arguments (A < 0, n < 1, k outside [2, 8], s outside [1, k - 1],
 *     min_gap < 1) or a total >= 2^63.
 * matcha_kway_anchor_rows   anchors device int64 [A, s]; writes x, device int64 [count, L] with k <= L <= 8, and flag, device int32
 *     [count] (non-zero = invalid; the layout matcha_hashset_contains writes, so the two can be OR-ed): row i is the candidate of
 *     global rank rank0 + i (ranks == NULL; the range must lie inside [0, A C_f), else refused) or ranks[i] (device int64 [count];
 *     a rank outside [0, A C_f) gives an all-zero row with its flag set).  One 64-bit division per row; count = 0 launches nothing.
 *
 * Segmented streaming selection: for each of A segments of seg_len consecutive global ranks, the best K (score, rank) pairs under
 * exactly the order of matcha_topk_* (NaN scores and skipped rows never kept, the stored score keeps its bits).  The state covers
 * the segments seg0 .. seg0 + A - 1, i.e. the ranks [seg0 seg_len, (seg0 + A) seg_len); the segment of a row is rank / seg_len.
 * A chunk may begin and end inside a segment and cover a fraction of one or thousands of them.  No atomics: the state after any
 * sequence of updates depends only on the pairs seen; segments a chunk does not touch are neither read nor written.
 * matcha_segtopk_bytes   bytes of one state (1 <= K, 1 <= A, A K < 2^31, seg_len >= 1, 1 <= max_chunk < 2^31); 0 when out of range.
 *     Sized without asking the device.  A, K, seg_len and max_chunk are passed again to the other three calls.
 * matcha_segtopk_init    empties every segment (a kernel, no memset).
 * matcha_segtopk_update  scores device float32 [n], row i has global rank g0 + i; skip optional device int32 [n]; 0 <= n <=
 *     max_chunk, n = 0 is a no-op that launches nothing; a range outside the state's segments is refused.
 * matcha_segtopk_read    scores_out device float32 [A, K], ranks_out device int64 [A, K] (global ranks), each segment sorted in the
 *     order above; counts_out device int64 [A]: the valid pairs of each segment (entries beyond are score 0, rank -1).
 * All refuse, before any device call: a null pointer, an argument out of range, a state smaller than matcha_segtopk_bytes. */
int64_t matcha_kway_anchor_count(int64_t A, int32_t s, int32_t n, int32_t k, int32_t min_gap);
int matcha_kway_anchor_rows(const int64_t* anchors, int64_t A, int32_t s, int64_t lo, int32_t n, int32_t k, int32_t min_gap,
                            int64_t rank0, const int64_t* ranks, int64_t count, int32_t L, int64_t* x, int32_t* flag,
                            matcha_stream_t stream);
size_t matcha_segtopk_bytes(int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk);
int matcha_segtopk_init(void* state, size_t bytes, int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk, matcha_stream_t stream);
int matcha_segtopk_update(void* state, size_t bytes, int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk, int64_t seg0,
                          const float* scores, const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream);
int matcha_segtopk_read(const void* state, size_t bytes, int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk, float* scores_out,
                        int64_t* ranks_out, int64_t* counts_out, matcha_stream_t stream);

/* ---- cluster completion -------------------------------------------------------------------------------
 * Which further bins best extend clusters of 1 to 31 loci: the anchored sweep's candidates for ragged anchors and rows of up to
 * MATCHA_MAX_LONG_L columns.  A cluster table is int64 [A, S], 1 <= S <= 31; row a holds s_a non-zero node ids followed by zeros,
 * 0 <= s_a <= S: the leading non-zero run is read, entries behind the first zero are ignored.  The free part is a candidate of size
 * f, 1 <= f <= 8, of the partner region [lo, lo + n) under the rule above (C_f values, ranked lexicographically from 0); the global
 * rank is g = a C_f + r, 0 <= g < A C_f < 2^63.  The candidate is the s_a + f ids sorted ascending (duplicates kept), zero-padded to
 * L, S + f <= L <= 32.  It is valid iff s_a >= 1, the cluster's own ids are non-descending and every adjacent difference is
 * >= min_gap.  Invalid candidates keep their rank and their row; a flag marks them.  A row with s_a = 0 is the free part alone,
 * flagged; a cluster row that descends somewhere leaves unmerged (its ids in their order, then the free ids), flagged.
 * matcha_kway_complete_count  host only: A C_f, or -1 for invalid arguments (A < 0, S outside [1, 31], n < 1, f outside [1, 8],
 *     min_gap < 1) or a total >= 2^63.
 * matcha_kway_complete_rows   clusters device int64 [A, S]; writes x, device int64 [count, L], and flag, device int32 [count]
 *     (non-zero = invalid): row i is the candidate of global rank rank0 + i (ranks == NULL; the range must lie inside [0, A C_f),
 *     else refused) or ranks[i] (device int64 [count]; a rank outside [0, A C_f) gives an all-zero row with its flag set).
 *     count = 0 launches nothing.  Every refusal is MATCHA_EINVAL with a message, before any device call; caller-owned memory,
 *     asynchronous on the caller's stream, no allocation, no memset, no read-back.  Selection: matcha_segtopk_* with seg_len = C_f. */
int64_t matcha_kway_complete_count(int64_t A, int32_t S, int32_t n, int32_t f, int32_t min_gap);
int matcha_kway_complete_rows(const int64_t* clusters, int64_t A, int32_t S, int64_t lo, int32_t n, int32_t f, int32_t min_gap,
                              int64_t rank0, const int64_t* ranks, int64_t count, int32_t L, int64_t* x, int32_t* flag,
                              matcha_stream_t stream);

/* ---- multi-region sweep --------------------------------------------------------------------------------
 * Candidates whose bins are drawn from several regions.  A sweep is P parts, 1 <= P <= 8, given as three HOST arrays of P elements
 * that are read before the call returns: part p is the region [lo[p], lo[p] + n[p]) of node ids and m[p] >= 1 bins drawn from it;
 * k = sum m[p], 2 <= k <= 8.  The regions are ascending and pairwise disjoint (lo[0] >= 0, lo[p] + n[p] <= lo[p + 1]).  A candidate
 * is the concatenation, part by part, of one candidate of every part under the rule above (C_p = C(n_p - (m_p - 1)(min_gap - 1),
 * m_p) of them, ranked r_p lexicographically from 0); the global rank is the mixed radix g = ((r_0 C_1 + r_1) C_2 + ...) C_{P-1} +
 * r_{P-1}, 0 <= g < T = prod C_p < 2^63.  Every row is ascending as it stands and rank order is the lexicographic order of the rows;
 * with P = 1 the rows are matcha_kway_rows'.  A candidate is invalid iff for some p the first id of part p + 1 minus the last id of
 * part p is below min_gap (two regions closer than min_gap); it keeps its rank and its row, a flag marks it.
 * matcha_kway_region_count  host only: T, or -1 for invalid arguments or T >= 2^63.
 * matcha_kway_region_rows   matcha_kway_anchor_rows' contract: writes x, device int64 [count, L] with k <= L <= 8 (columns k .. L - 1
 *     zero), and flag, device int32 [count] (non-zero = invalid): row i is the candidate of global rank rank0 + i (ranks == NULL; the
 *     range must lie inside [0, T), else refused) or ranks[i] (device int64 [count]; a rank outside [0, T) gives an all-zero row with
 *     its flag set).  At most one division per part and row.  count = 0 launches nothing.  Every refusal (P outside [1, 8], an m[p] or
 *     n[p] < 1, k outside [2, 8], min_gap < 1, regions not ascending and disjoint, a lo out of range, T >= 2^63, a range outside
 *     [0, T), count out of range, a null pointer) is MATCHA_EINVAL with a message, before any device call; caller-owned memory,
 *     asynchronous on the caller's stream, no allocation, no memset, no read-back.  Selection: matcha_topk_*, or matcha_segtopk_* with
 *     seg_len = T / C_0 for the best K per candidate of the leading part. */
int64_t matcha_kway_region_count(int32_t P, const int64_t* lo, const int32_t* n, const int32_t* m, int32_t min_gap);
int matcha_kway_region_rows(int32_t P, const int64_t* lo, const int32_t* n, const int32_t* m, int32_t min_gap, int64_t rank0,
                            const int64_t* ranks, int64_t count, int32_t L, int64_t* x, int32_t* flag, matcha_stream_t stream);

/* ---- cluster growth -------------------------------------------------------------------------------------
 * A beam search that grows hubs of up to 32 loci from seed clusters, one bin of the region [lo, lo + n) per step.  The beam table is
 * int64 [A, B, S]: A seeds, B slots per seed (1 <= B <= 64), each slot a cluster row of matcha_kway_complete_rows (1 <= S <= 31, the
 * leading non-zero run; an all-zero slot is empty).  Entry e = a B + j; the candidate of (e, r) is that of cluster e with f = 1 and
 * free id lo + r, its global rank g = e n + r, 0 <= g < A B n < 2^63: rows, validity and flag bit 1 come from
 * matcha_kway_complete_rows(beam, A B, S, lo, n, 1, min_gap, ...).  Candidate (a, j, r) is a TWIN iff a lower slot j' < j of the same
 * seed is strictly ascending, non-empty, holds as many ids as slot j (strictly ascending too) and slot_j' \ slot_j is {lo + r} or
 * empty (identical slots: every candidate of slot j is a twin).  Of all candidates of a seed that give the same sorted row exactly
 * one is not a twin: the one of the lowest slot.  Selection: matcha_segtopk_* with seg_len = B n.
 * matcha_grow_twins       beam device int64 [A, B, S]; writes twin, device int64 [A B, B]: column j' < j of row e = a B + j holds
 *     the one id of slot_j' \ slot_j, -1 for identical slots, 0 for no relation; columns j' >= j are 0.  A = 0 launches nothing.
 * matcha_grow_twin_flags  ORs 2 into flag[i] (device int32 [count], as matcha_kway_complete_rows wrote it) when the candidate of
 *     global rank rank0 + i is a twin: lo + r stands in its entry's twin row, or a -1 does.  The range must lie inside [0, A B n),
 *     else refused; count = 0 or A = 0 launches nothing.
 * Both: every refusal (B outside [1, 64], S outside [1, 31], n < 1, A < 0, lo < 0, A B n >= 2^63, a null pointer) is MATCHA_EINVAL
 * with a message, before any device call; caller-owned memory, asynchronous on the caller's stream, no allocation, no memset, no
 * read-back. */
int matcha_grow_twins(const int64_t* beam, int64_t A, int32_t B, int32_t S, int64_t* twin, matcha_stream_t stream);
int matcha_grow_twin_flags(const int64_t* twin, int64_t A, int32_t B, int64_t lo, int32_t n, int64_t rank0, int64_t count, int32_t* flag,
                           matcha_stream_t stream);

/* ---- cluster decomposition ----------------------------------------------------------------------------
 * Which sub-hyperedges of clusters of up to 32 loci are real (keep), and which locus does not belong (drop): the candidates are
 * subsets of a cluster's OWN ids.  A cluster table is int64 [A, S], 2 <= S <= 32; row a holds s_a non-zero node ids followed by
 * zeros: the leading non-zero run is read.  A choice is an m-subset of the positions [0, S), 1 <= m <= 8, ranked lexicographically
 * from 0 (C_m = C(S, m) <= C(32, 8) of them); the global rank is g = a C_m + r.  complement = 0 (keep, 2 <= m <= 8): the row is the
 * ids at the chosen positions; complement = 1 (drop, 1 <= m <= 8): the ids at every other position; both in position order,
 * zero-padded to L (keep: m <= L <= 32; drop: max(S - m, 1) <= L <= 32).  A candidate is valid iff every chosen position is < s_a,
 * the row has at least 2 ids, the cluster's ids are non-descending and every adjacent difference of the row is >= min_gap.  A
 * candidate with a chosen position >= s_a is an all-zero row with its flag set; every other invalid candidate keeps its row.
 * matcha_cluster_subset_count  host only: A C(S, m), or -1 for invalid arguments or a total >= 2^63.
 * matcha_cluster_subset_rows   matcha_kway_complete_rows' contract: clusters device int64 [A, S]; writes x, device int64 [count, L],
 *     and flag, device int32 [count] (non-zero = invalid): row i is the candidate of global rank rank0 + i (ranks == NULL; the range
 *     must lie inside [0, A C_m), else refused) or ranks[i] (device int64 [count]; a rank outside [0, A C_m) gives an all-zero row
 *     with its flag set).  count = 0 launches nothing.  Every refusal is MATCHA_EINVAL with a message, before any device call;
 *     caller-owned memory, asynchronous on the caller's stream, no allocation, no memset, no read-back.
 * matcha_subset_support_*      per cluster and position, what a top-K cannot give: over the accepted rows whose choice contains the
 *     position, the sum of their values in PairMap's fixed point (int64, rint(double(v) 2^32)) and their number; two int64 planes
 *     [A, S] behind a 256-byte header {n_rows, n_rejected}.  1 <= A <= 2^40, 0 < vmax <= 2^20.  _bytes: the state's size, 0 for
 *     invalid arguments.  _init zeroes the state (a kernel, no memset).  _update: value device float32 [n], skip device int32 [n] or
 *     NULL; row i has the global rank g0 + i (the range must lie inside [0, A C_m)) and its choice is unranked on the device -- no row
 *     is read; a row with skip != 0 contributes nothing, one whose value is NaN, negative or > vmax is counted in n_rejected.
 *     Integer atomics only: the state is bit for bit independent of arrival order and of how the stream is cut.  _read: the planes
 *     (device int64 [A, S]) and the two counters (device int64 [2]); any of the three may be NULL, not all.
 * matcha_subset_pair_*         per cluster and PAIR of positions i < j: over the accepted rows whose choice contains
 *     both, the same fixed-point sum and their number.  matcha_subset_support_*'s arguments, checks, refusals and row handling, except
 *     2 <= m <= 8 (a choice of one position has no pair).  State: the 256-byte header {n_rows, n_rejected}, then two planes of A P
 *     cells, P = S (S - 1) / 2, each padded to a multiple of 256 bytes: the upper triangle only, row-major; the cell of positions
 *     i < j of cluster a is a P + i (2 S - i - 1) / 2 + (j - i - 1).  An accepted row adds rint(double(v) 2^32) and 1 to the C(m, 2)
 *     cells of its choice.  Like the support planes, a cell holds count * v * 2^32 modulo 2^64: exact while its true sum stays below
 *     2^31.  Integer atomics only: the state, header and padding included, is bit for bit independent of arrival order and of how the
 *     ranks are cut into calls.  _read: the packed planes (device int64 [A, P]) and the two counters; any may be NULL, not all. */
int64_t matcha_cluster_subset_count(int64_t A, int32_t S, int32_t m, int32_t complement);
int matcha_cluster_subset_rows(const int64_t* clusters, int64_t A, int32_t S, int32_t m, int32_t complement, int32_t min_gap,
                               int64_t rank0, const int64_t* ranks, int64_t count, int32_t L, int64_t* x, int32_t* flag,
                               matcha_stream_t stream);
size_t matcha_subset_support_bytes(int64_t A, int32_t S, int32_t m, float vmax);
int matcha_subset_support_init(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, matcha_stream_t stream);
int matcha_subset_support_update(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, const float* value,
                                 const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream);
int matcha_subset_support_read(const void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, int64_t* sum_out,
                               int64_t* count_out, int64_t* counters_out, matcha_stream_t stream);
size_t matcha_subset_pair_bytes(int64_t A, int32_t S, int32_t m, float vmax);
int matcha_subset_pair_init(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, matcha_stream_t stream);
int matcha_subset_pair_update(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, const float* value,
                              const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream);
int matcha_subset_pair_read(const void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, int64_t* sum_out,
                            int64_t* count_out, int64_t* counters_out, matcha_stream_t stream);

/* ---- k-way pair maps -----------------------------------------------------------------------------------
 * The values of k-way rows projected onto pairs of node ids and accumulated on the device.  A map covers the row region
 * R = [lo_r, lo_r + n_r) and the column region C = [lo_c, lo_c + n_c): R == C (symmetric) or R and C disjoint (rectangular); any
 * other overlap, n_r n_c >= 2^31, an empty or unknown plane mask and a vmax outside (0, 2^20] are refused.
 * Row i of an update (x device int64 [n, L], 2 <= L <= 8, 0 = padding; value device float32 [n]; skip optional device int32 [n],
 * the layout matcha_hashset_contains and matcha_kway_anchor_rows write) contributes nothing when skip[i] != 0 (not counted), or
 * when value[i] is NaN, < 0 or > vmax (counted in n_rejected; -0.0 is accepted as 0, +inf is rejected).  Every other row counts in
 * n_rows and contributes value[i] once for each pair of positions ci < cj with a = x[ci], b = x[cj] both non-zero, a != b, and
 *   rectangular: cell (a - lo_r, b - lo_c) if a in R and b in C, else (b - lo_r, a - lo_c) if b in R and a in C, else none;
 *   symmetric:   cell (min(a, b) - lo, max(a, b) - lo) if both are in R, else none (the read mirrors it; the diagonal reads 0).
 * Rows need not be sorted or duplicate-free: (5, 5, 9) adds twice to {5, 9}.
 * Planes (a bit mask; only the planes asked for take memory):
 *   MATCHA_PAIRMAP_SUM       int64, the sum of rint((double)v * 2^32): fixed point with 32 fractional bits (exact for v >= 2^-8),
 *                            so the plane is bitwise independent of arrival order and of how the stream is cut into updates.
 *                            Exact while a cell's true sum stays below 2^31; capacity is the caller's to declare.
 *   MATCHA_PAIRMAP_COUNT     int64, the number of contributions.
 *   MATCHA_PAIRMAP_COUNT_GE  int64, the number of contributions with v >= threshold (compared in float32).
 *   MATCHA_PAIRMAP_MAX       float32, the largest contributing v (-inf in a cell never hit).
 * State blob (caller-owned, 8-byte aligned, matcha_pairmap_bytes bytes): a 256-byte header {int64 n_rows, int64 n_rejected, zero
 * padding}, then the planes present in the order SUM, COUNT, COUNT_GE (n_r n_c int64 each), MAX (n_r n_c uint32 keys: 0 = never
 * hit, else the float's bits | 0x80000000), every plane row-major [n_r][n_c] and padded to a multiple of 256 bytes; a symmetric map
 * only ever writes its upper triangle.  The regions, the mask, vmax and threshold are passed to every call: the library keeps nothing
 * on the host between calls, never allocates and never reads the state back; all calls are asynchronous on the caller's stream.
 * matcha_pairmap_bytes   host only; 0 for invalid arguments.
 * matcha_pairmap_init    zeroes the state (a kernel, no memset).
 * matcha_pairmap_update  n = 0 is a no-op that launches nothing.  Integer atomics only: every plane is deterministic.
 * matcha_pairmap_read    plane = ONE bit of the mask; out device int64 [n_r, n_c] (the raw fixed-point sums for SUM) or float32
 *     [n_r, n_c] for MAX; counters_out optional device int64 [2] = {n_rows, n_rejected}.
 * All refuse, before any device call: a null pointer, arguments out of range, L outside [2, 8], n < 0, a state that is too small. */
#define MATCHA_PAIRMAP_SUM 1
#define MATCHA_PAIRMAP_COUNT 2
#define MATCHA_PAIRMAP_COUNT_GE 4
#define MATCHA_PAIRMAP_MAX 8
size_t matcha_pairmap_bytes(int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes, float vmax, float threshold);
int matcha_pairmap_init(void* state, size_t bytes, int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes, float vmax,
                        float threshold, matcha_stream_t stream);
int matcha_pairmap_update(void* state, size_t bytes, int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes, float vmax,
                          float threshold, const int64_t* x, const float* value, const int32_t* skip, int64_t n, int32_t L,
                          matcha_stream_t stream);
int matcha_pairmap_read(const void* state, size_t bytes, int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes,
                        float vmax, float threshold, int32_t plane, void* out, int64_t* counters_out, matcha_stream_t stream);

/* ---- distance-matched expectation of k-way sweeps (csrc/expected.hip) ----
 * A candidate of size k is a strictly ascending k-tuple of positive node ids, zero-padded to the row width L (2 <= k <= L <= 8).  Its gaps
 * g_j = x[j+1] - x[j] fall into classes: class(g) = the number of edges <= g, `edges` a strictly ascending host array of 0 .. 15 positive
 * int64 (copied into the kernel arguments: the library keeps nothing between calls), G = n_edges + 1 classes.  The stratum is
 * s = ((c_0 G + c_1) G + ...) + c_{k-2} in [0, G^(k-1)), G^(k-1) <= 2^20; gap tuples stay ordered.  A row whose leading non-zero run is not
 * exactly k ids, is not strictly ascending, starts below 1 or holds a non-zero id behind a zero has stratum -1.
 * Statistics (a bit mask of planes, int64 [G^(k-1)] each; only the planes asked for take memory): an accepted row -- skip[i] == 0, stratum
 * >= 0, 0 <= v <= vmax (-0.0 counts as 0; everything else that is not skipped is counted in n_rejected) -- adds
 *   MATCHA_GAP_COUNT  1,      MATCHA_GAP_SUM  rint((double)v 2^shift),      MATCHA_GAP_SUMSQ  rint((double)v (double)v 2^shift)
 * to its stratum with integer adds, so every plane is bitwise independent of the order of the rows and of how the stream is cut.
 * MATCHA_GAP_DIRECT in the mask of an update (ignored elsewhere) turns the block-level accumulation in LDS off: an A/B switch, same planes.
 * State blob (caller-owned, 8-byte aligned, exactly matcha_gap_stats_bytes bytes): a 256-byte header {int64 n_rows, int64 n_rejected, zero
 * padding}, then the planes present in the order COUNT, SUM, SUMSQ, each padded to a multiple of 256 bytes.  All calls are asynchronous on
 * the caller's stream; nothing is allocated or read back.
 * matcha_gap_strata_count  host only: G^(k-1), or -1 for k outside [2, 8], n_edges outside [0, 15] or more than 2^20 strata.
 * matcha_gap_strata_ids    stratum_out device int32 [n].
 * matcha_gap_stats_bytes   host only; 0 for invalid arguments.
 * matcha_gap_stats_init    zeroes the state (a kernel, no memset).
 * matcha_gap_stats_update  x device int64 [n, L], value device float32 [n], skip device int32 [n] or null; n = 0 launches nothing.  16 <= shift
 *     <= 32, 0 < vmax <= 2^20, and with SUMSQ vmax^2 2^shift <= 2^62 (one row's term must fit).
 * matcha_gap_stats_read    the raw planes to device int64 [G^(k-1)] arrays (null = not wanted; a non-null output needs its plane in the mask),
 *     counters_out optional device int64 [2] = {n_rows, n_rejected}.
 * matcha_gap_enrich        out[i] = (score[i] - offset[s]) * scale[s], two separately rounded float32 operations (no FMA), NaN for stratum -1;
 *     offset, scale device float32 [G^(k-1)]; stratum_out optional device int32 [n].  With score, offset, scale and out all null only the
 *     strata are written.
 * All refuse with MATCHA_EINVAL, before any device call: k outside [2, 8], L < k or L > 8, more than 15 edges, edges not positive and strictly
 * ascending, more than 2^20 strata, an empty or unknown plane mask, shift or vmax out of range, a `bytes` that differs from the sizing call,
 * null pointers, n < 0. */
#define MATCHA_GAP_COUNT 1
#define MATCHA_GAP_SUM 2
#define MATCHA_GAP_SUMSQ 4
#define MATCHA_GAP_DIRECT 8
int64_t matcha_gap_strata_count(int32_t k, int32_t n_edges);
int matcha_gap_strata_ids(int32_t k, const int64_t* edges, int32_t n_edges, const int64_t* x, int64_t n, int32_t L, int32_t* stratum_out,
                          matcha_stream_t stream);
size_t matcha_gap_stats_bytes(int32_t k, int32_t n_edges, int32_t planes);
int matcha_gap_stats_init(void* state, size_t bytes, int32_t k, int32_t n_edges, int32_t planes, matcha_stream_t stream);
int matcha_gap_stats_update(void* state, size_t bytes, int32_t k, const int64_t* edges, int32_t n_edges, int32_t planes, int32_t shift, float vmax,
                            const int64_t* x, int32_t L, const float* value, const int32_t* skip, int64_t n, matcha_stream_t stream);
int matcha_gap_stats_read(const void* state, size_t bytes, int32_t k, int32_t n_edges, int32_t planes, int64_t* count_out, int64_t* sum_out,
                          int64_t* sumsq_out, int64_t* counters_out, matcha_stream_t stream);
int matcha_gap_enrich(int32_t k, const int64_t* edges, int32_t n_edges, const int64_t* x, int64_t n, int32_t L, const float* score,
                      const float* offset, const float* scale, int32_t* stratum_out, float* out, matcha_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MATCHA_HIP_H */
