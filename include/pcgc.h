/*
 * pcgc.h — C ABI of the MI355X-native PCGCv1 hot path.
 *
 * Two shared libraries implement it:
 *   libpcgc_hip.so   (hipcc, gfx950)  every pcgc_* function that takes a stream
 *   libpcgc_host.so  (g++)            the sequential host tail: range coder, CDF
 *                                      quantiser, partition / merge, ply text
 *
 * The reference is pure Python on TensorFlow 1.13; its "FFI" for this path is
 * the set of TF ops its Python calls.  Each entry point below names the
 * reference call site it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - extern "C"; every function returns int: 0 = ok, < 0 = error
 *     (pcgc_last_error() / pcgc_host_last_error() give a thread-local message).
 *   - Caller owns every buffer.  Device pointers are plain pointers obtained
 *     from any HIP allocator (the Python host passes torch allocations).
 *     Device memory the library allocates itself: the weight copy inside a pcgc_net
 *     (freed by pcgc_net_destroy), a stream-ordered temporary for the repacked weights of a
 *     single pcgc_conv3d_fwd call on a matrix-core shape (hipMallocAsync / hipFreeAsync on the
 *     caller's stream), and one 512 KiB log2 table per device (first pcgc_laplace_cdf call).
 *     Everything else comes from the caller, sized by the *_workspace_bytes functions.
 *   - Every device function enqueues on the caller's stream (hipStream_t passed
 *     as void*), asynchronously, with no hidden synchronisation.
 *   - Activations are NDHWC float32, contiguous.  Weights are passed in
 *     TensorFlow layouts: Conv3D [kd,kh,kw,Cin,Cout], Conv3DTranspose
 *     [kd,kh,kw,Cout,Cin] (models/model_voxception.py:21-54, 164-182).
 *   - Empty inputs (B = 0 cubes / n = 0 elements / rows = 0) are valid no-ops of the forward, likelihood, CDF and
 *     top-k entry points: they return 0 without touching any pointer (which may then be NULL).
 *   - No floating-point atomics and no grid-size-dependent reduction order
 *     anywhere: results are bit-identical for any batch size / batch slot /
 *     GPU count (the reference's known enc/dec mismatch, README.md:111-114).
 */
#ifndef PCGC_H_
#define PCGC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pcgc_stream_t; /* hipStream_t */

/* ------------------------------------------------------------------ */
/* libpcgc_hip.so                                                      */
/* ------------------------------------------------------------------ */
int pcgc_version(void);
const char* pcgc_last_error(void);

/* One Keras Conv3D / Conv3DTranspose (padding='same') + bias + optional ReLU.
 * Replaces tf.keras.layers.Conv3D/Conv3DTranspose.__call__
 * (models/model_voxception.py:21-54, 83-122, 153-192, 224-244, 263-297).
 *   x [B,D,D,D,Cin] -> y [B,Do,Do,Do,Cout];  Do = D (stride 1), D/2 (stride 2),
 *   2D (transposed).  ksize odd, 1..9 (3 and 1 in model_voxception.py, 5 and 9 in model_simple.py:20-41, 56-86:
 *   those run on the generic direct kernel); stride 1 or 2; transposed implies stride 2.  TF 'SAME' padding: a
 *   stride-2 conv pads ksize-2 voxels in total, the smaller half in front; the transposed conv is its adjoint.
 *   bias may be NULL (down_1/down_2, model_voxception.py:99,111).
 *   algo: 0 = auto (MFMA kernel when the shape has one, else direct),
 *         1 = force the direct (VALU) kernel, 2 = force MFMA (error if none). */
int pcgc_conv3d_fwd(const float* x, const float* kernel, const float* bias, float* y,
                    int B, int D, int Cin, int Cout, int ksize, int stride,
                    int transposed, int relu, int algo, pcgc_stream_t stream);

/* One _VoxceptionResNet block (model_voxception.py:11-68, call 56-68):
 *   out = relu(x + concat[ relu(conv1_2(relu(conv1_1(x)))),
 *                          relu(conv2_3(relu(conv2_2(relu(conv2_1(x)))))) ])
 * x, out: [B, D, D, D, C] NDHWC fp32 (out may alias x).  params = the block's ten tensors in the
 * order of its layers {conv1_1, conv1_2, conv2_1, conv2_2, conv2_3}, kernel then bias each, kernels in
 * the Keras layout [kd,kh,kw,Cin,Cout].  C = 16 at D = 64, C = 32 at D = 32 and C = 64 at D = 16 (the three stages
 * of both transforms) run the v_mfma_f32_4x4x1 row kernels that pcgc_net_forward uses for those stages;
 * any other C % 4 == 0 runs the generic layer kernels.  Workspace from pcgc_vrn_workspace_bytes. */
size_t pcgc_vrn_workspace_bytes(int B, int D, int C);
int pcgc_vrn_fwd(const float* x, const float* const* params, float* out, int B, int D, int C,
                 void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* Whole transforms.  kind selects the layer table (pcgcv1_amd/models/spec.py,
 * restating model_voxception.py:71-308). */
enum {
  PCGC_NET_ANALYSIS = 0,      /* AnalysisTransform.call   model_voxception.py:125-144 */
  PCGC_NET_SYNTHESIS = 1,     /* SynthesisTransform.call  model_voxception.py:195-214 */
  PCGC_NET_HYPER_ENCODER = 2, /* HyperEncoder.call        model_voxception.py:246-252 */
  PCGC_NET_HYPER_DECODER = 3  /* HyperDecoder.call        model_voxception.py:299-308 */
};
typedef struct pcgc_net pcgc_net;

/* Number of parameter tensors `params` must hold for `kind`: for every layer of
 * the table, in order, its kernel then (if the layer has one) its bias. */
int pcgc_net_param_count(int kind);
/* params[i] are DEVICE pointers in TF layouts; they are repacked into the
 * library's MFMA operand layout on `stream`; the caller may free them after
 * synchronising the stream.  Replaces tf.train.Checkpoint.restore binding
 * (transform.py:107-112, 214-218). */
int pcgc_net_create(int kind, const float* const* params, int n_params,
                    pcgc_stream_t stream, pcgc_net** out);
void pcgc_net_destroy(pcgc_net* net);
/* algo 0 (default): MFMA kernels wherever a shape has one; 1: direct (VALU) kernels only
 * (the on-device cross-check the parity tests use). */
int pcgc_net_set_algo(pcgc_net* net, int algo);
/* Exact skipping of empty space (AnalysisTransform at cube size 64; model_voxception.py:125-131 = conv_in + the three
 * C = 16 blocks).  A 64^3 cube of a voxelised surface is ~98 % zeros; wherever the receptive field of a wave tile of a
 * layer's output holds no occupied voxel the tile equals, bit for bit, the same tile of that layer's response to an
 * all-zero cube (kept per net, made by the same kernels at pcgc_net_create), and the wave copies it instead of computing
 * it.  Results are identical with and without (environment PCGC_SKIP_EMPTY=0 computes every tile).
 * PCGC_SKIP_EMPTY=3 (the default): conv_in and the three C = 16 blocks work on SLOTS of 8 planes x 2 rows x 16 voxels instead
 * of whole-row tiles — four slots to a wave, only the heavy ones launched, a slot nobody wrote read from the empty-cube
 * response by its reader (csrc/vrn_seg.hip); 1: whole-row tiles that are not written, 2: whole-row tiles that are copied.
 * The workspace (pcgc_net_workspace_bytes) then also holds the slot lists and room for a copy of the empty-cube responses,
 * which is made only when the net's own copy and the chunk's tensors do not fit one 2 GiB buffer window.
 * pcgc_rowocc: rowocc[b * 64 + d] bit h = row (d, h) of cube b holds a voxel that is not +0.0 — what the row-tile forms test.
 * pcgc_net_set_skip_counter: test aid — a device word that receives +1 per skipped wave tile / slot (NULL: off). */
int pcgc_rowocc(const float* x, unsigned long long* rowocc, int B, pcgc_stream_t stream);
int pcgc_net_set_skip_counter(pcgc_net* net, unsigned* device_counter);
/* Per-launch timing for bench.py's roofline line: when on, every layer launch of pcgc_net_forward is
 * bracketed by hipEvents on the caller's stream.  pcgc_net_profile_report drains them as text, one line per
 * launch: "layer_index layer_name mfma|direct Cin Cout k mode B Din milliseconds".  Call with buf = NULL to
 * get the size in *needed (the records are consumed by the call that copies them). */
int pcgc_net_set_profiling(pcgc_net* net, int on);
int pcgc_net_profile_report(pcgc_net* net, char* buf, size_t cap, size_t* needed);
/* Scratch the forward pass needs for a batch of B cubes whose INPUT spatial
 * size is D (64 for analysis, 16 for synthesis / hyper encoder, 8 for hyper
 * decoder at cube_size 64). */
size_t pcgc_net_workspace_bytes(const pcgc_net* net, int B, int D);
/* Forward pass.  out1 is only used by the hyper decoder: out0 = loc,
 * out1 = max(|scale|, scale_lower_bound)  (model_voxception.py:308 +
 * transform.py:145-146, 232-233; train_hyper.py:189).
 * Replaces tf.map_fn(loop_analysis | loop_synthesis | loop_hyper_*),
 * transform.py:116-147, 224-257 — batched instead of one cube per call. */
int pcgc_net_forward(const pcgc_net* net, const float* x, float* out0, float* out1,
                     int B, int D, float scale_lower_bound, void* workspace,
                     size_t workspace_bytes, pcgc_stream_t stream);

/* ---- entropy-model kernels -------------------------------------------- */

/* tf.math.round (half-to-even) of n floats + per-segment min / max of the
 * rounded values (segments = consecutive runs of seg_len elements).
 * Replaces _quantize(..., "symbols") + reduce_min/max,
 * conditional_entropy_model.py:151-154 (per cube) and entropy_model.py:246-250
 * (one segment = whole batch).  q may be NULL.  seg_min/seg_max: int32[n/seg_len]. */
int pcgc_repro_eval(int fn, const float* x, float* y, int64_t n, pcgc_stream_t stream);

int pcgc_round_minmax(const float* x, float* q, int32_t* seg_min, int32_t* seg_max,
                      int64_t n, int64_t seg_len, pcgc_stream_t stream);
/* The same with the rounded values as int16 — the coder's input type (entropy_model.py:253-258: cast, - min_v, cast to int16,
 * range_encode): no float tensor, no conversion pass.  Values outside 16 bits saturate; the caller reads seg_min / seg_max
 * anyway and refuses such a range. */
int pcgc_round_minmax_i16(const float* x, int16_t* q, int32_t* seg_min, int32_t* seg_max,
                          int64_t n, int64_t seg_len, pcgc_stream_t stream);
/* Decoder side of the same cast (entropy_model.py:298-304: range_decode -> + min_v -> float32):
 * out[i] = (float)sym[i] + offset. */
int pcgc_symbols_to_values(const int16_t* sym, int offset, float* out, int64_t n, pcgc_stream_t stream);
/* Per-cube form (conditional_entropy_model.py:195-199: each cube's decoded symbols + that cube's min_v):
 * out[i] = (float)sym[i] + seg_offset[i / seg_len], seg_offset float32 [n / seg_len] on the device. */
int pcgc_symbols_to_values_seg(const int16_t* sym, const float* seg_offset, float* out, int64_t n, int64_t seg_len,
                               pcgc_stream_t stream);

/* SymmetricConditional.__call__ (conditional_entropy_model.py:71-93), eval or
 * training (noise = U(-.5,.5) supplied by the caller, may be NULL for eval):
 * values = round(y) or y+noise; likelihood = max(|c(up')-c(lo')|, bound). */
int pcgc_laplace_likelihood(const float* y, const float* loc, const float* scale,
                            const float* noise, float* values, float* likelihood,
                            int64_t n, float likelihood_bound, pcgc_stream_t stream);

/* SymmetricConditional._get_cdf (conditional_entropy_model.py:95-124) fused with
 * pmf_to_quantized_cdf (TF 1.13 contrib/coder, call site :122) for `rows`
 * (voxel,channel) rows grouped in segments of seg_rows rows (one segment = one
 * cube); segment s uses the integer support [seg_min[s], seg_max[s]].
 *   cdf_lower: uint16 [rows, ncols]; entry k is the quantised CDF value at
 *              symbol k (cdf[0] = 0); the implicit entry past the last symbol
 *              is 65536.  ncols >= max over segments of (max-min+1).
 *   If symbols != NULL (float, already rounded) also writes
 *   lohi[row] = lower | (upper-1) << 16 for that row's symbol (what range_encode
 *   consumes, conditional_entropy_model.py:161).  Either output may be NULL.
 * The first call on a device allocates and uploads a 512 KiB table of log2(v), v in [0, 65536] (computed on the
 * host in double, like the oracle) and synchronises once; later calls are asynchronous on `stream`. */
int pcgc_laplace_cdf(const float* loc, const float* scale, const int32_t* seg_min,
                     const int32_t* seg_max, int64_t rows, int64_t seg_rows, int ncols,
                     float likelihood_bound, const float* symbols, uint16_t* cdf_lower,
                     uint32_t* lohi, pcgc_stream_t stream);

/* EntropyBottleneck.__call__ (entropy_model.py:153-181).  params: the 12 tensors
 * matrix_0,bais_0,factor_0,...,matrix_3,bais_3,factor_3 packed back to back
 * (C*(3+3+3 + 9+3+3 + 9+3+3 + 3+1+1) floats, entropy_model.py:50-66), device. */
int pcgc_factorized_likelihood(const float* z, const float* params, const float* noise,
                               float* values, float* likelihood, int64_t n, int C,
                               float likelihood_bound, pcgc_stream_t stream);
/* EntropyBottleneck._get_cdf pmf part (entropy_model.py:199-214): pmf [C, N] over
 * the integers min_v..max_v (device output). */
int pcgc_factorized_pmf(const float* params, int C, int min_v, int max_v,
                        float likelihood_bound, float* pmf, pcgc_stream_t stream);

/* ---- decoder tail ------------------------------------------------------ */
/* select_voxels + get_adaptive_thres (dataprocess/inout_points.py:147-179):
 * per cube b: k = k_per_cube[b]; threshold = k-th largest of the values > -2.0
 * (all values if fewer than k; k = 0 -> the smallest candidate); or
 * fixed_thres when use_fixed != 0.  Writes thresholds[b] and, if mask != NULL,
 * mask[b, v] = (x >= thres) as uint8.  vox = voxels per cube. */
int pcgc_topk_threshold(const float* x, const int32_t* k_per_cube, int B, int64_t vox,
                        int use_fixed, float fixed_thres, float* thresholds,
                        uint8_t* mask, void* workspace, size_t workspace_bytes,
                        pcgc_stream_t stream);
size_t pcgc_topk_workspace_bytes(int B, int64_t vox);

/* loss.get_bce_loss (loss.py:8-33): sums[0..3] = sum_{label=0} -log(1-o),
 * count(label=0), sum_{label>0} -log(o), count(label>0); o = clip(sigmoid(pred)).
 * Deterministic two-stage reduction (double). */
int pcgc_bce_sums(const float* pred, const float* label, int64_t n, double* sums4,
                  void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
size_t pcgc_bce_workspace_bytes(int64_t n);

/* loss.get_confusion_matrix / get_classify_metrics (loss.py:35-78).  pred, label: n floats; a voxel is positive
 * when its value is > th.  pcgc_classify_sums: sums3 = {TP, FP, FN} as exact counts (wavefront ballot + popcount,
 * fixed-order two-stage sum); precision = TP/(TP+FP), recall = TP/(TP+FN), IoU = TP/(TP+FP+FN) are formed by the
 * caller.  pcgc_confusion_matrix writes the three 0/1 maps TP = p*l, FP = p*(1-l), FN = (1-p)*l. */
size_t pcgc_classify_workspace_bytes(void);
int pcgc_classify_sums(const float* pred, const float* label, int64_t n, float th, double* sums3,
                       void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_confusion_matrix(const float* pred, const float* label, int64_t n, float th, float* tp,
                          float* fp, float* fn, pcgc_stream_t stream);

/* loss.get_focal_loss (loss.py:83-93): y_pred are probabilities, y_true is 0 / 1.
 *   loss = - sum alpha (1 - pt_1)^gamma log(pt_1) - sum (1 - alpha) pt_0^gamma log(1 - pt_0),
 *   pt_1 = clip(y_true == 1 ? y_pred : 1, 1e-3, .999), pt_0 = clip(y_true == 0 ? y_pred : 0, 1e-3, .999)
 * (float32 per element, wavefront butterfly + fixed-order double sum).  _bwd: dy_pred = grad_scale * dloss/dy_pred,
 * zero where y_pred is outside the clip range. */
size_t pcgc_focal_workspace_bytes(void);
int pcgc_focal_loss(const float* y_pred, const float* y_true, int64_t n, float gamma, float alpha, double* loss,
                    void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_focal_loss_bwd(const float* y_pred, const float* y_true, int64_t n, float gamma, float alpha,
                        float grad_scale, float* dy_pred, pcgc_stream_t stream);

/* D1 (point-to-point) distortion of MPEG pc_error as the reference's eval uses it
 * (myutils/pc_error_wrapper.py:26-75; eval.py:194-207): out2[0] = mean over the points of A of the squared
 * distance to the nearest point of B, out2[1] = the largest such squared distance (squared Hausdorff).
 * Points are int32 xyz with 0 <= coordinate < res.  Call twice (A->B, B->A); PSNR = 10 log10(3 peak^2 / max mse).
 * Exact (integer distances); deterministic. */
size_t pcgc_d1_workspace_bytes(int res);
int pcgc_d1_mse(const int32_t* pa, int64_t na, const int32_t* pb, int64_t nb, int res, double* out2,
                void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* D2 (point-to-plane) distortion of MPEG pc_error 0.13.4 (`-n normal1`, neighborsProc 1, averageNormals 1;
 * myutils/pc_error_wrapper.py:46-51).  The target cloud Q is passed as its linear keys (x*res + y)*res + z, int64,
 * SORTED ascending and unique; per-point arrays of Q (normals) are in that order.
 *   pcgc_d2_transfer_normals: normals_q[j] = mean of normals_p[i] over every i whose nearest-neighbour set in Q
 *     (all points at the minimal distance) contains j; zero where no point of P maps to j.
 *   pcgc_d2_mse: out2[0] = mean over p of mean_{q in T(p)} ((p-q).normal_q)^2, out2[1] = the largest such value.
 * Deterministic (integer atomics / fixed-order double sums). */
size_t pcgc_d2_workspace_bytes(int res, int64_t nq);
int pcgc_d2_transfer_normals(const int32_t* p, int64_t np, const float* normals_p, const int64_t* qkeys, int64_t nq,
                             int res, float* normals_q, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_d2_mse(const int32_t* p, int64_t np, const int64_t* qkeys, int64_t nq, const float* normals_q, int res,
                double* out2, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* D1 / D2 of pc_error between clouds that are NOT on the integer grid: float32 xyz, integral or not (a reconstruction
 * scaled back by 1 / scale; any two clouds that were never voxelised).  All distances are float64 arithmetic on the
 * coordinates as they are: d2(p, q) = (dx*dx + dy*dy) + dz*dz with dx = double(p.x) - double(q.x), in this association.
 * The target cloud Q is bucketed into cubic cells of edge h, a power of two within [1, 2^20]:
 *   cell = floor(q / h) - (ox, oy, oz), each component within [0, res), res <= 1024, |o| < 2^29,
 * and is passed SORTED ascending by the cell key (cx*res + cy)*res + cz (any number of points per cell, in any order
 * within one; that order is the order of the plane sums); per-point arrays of Q are in that order.  P may lie anywhere,
 * also outside Q's grid, as long as |floor(p / h) - o| < 2^29.  best(p) = min over Q of d2; the search walks Chebyshev
 * shells of cells around p's cell and stops after shell w once best + 1e-8 <= (w h)^2.  T(p) = EVERY q with
 * |d2(p, q) - best(p)| < 1e-8 (pc_error's tie rule, absolute on squared distances; no cap on their number).
 *   pcgc_offgrid_transfer_normals: normals_q[j] (double [nq,3]) = mean of normals_p[i] (float32) over every i with j in
 *     T(p_i), as sum of llrint(n * 2^40) in int64 / 2^40 / count; zero where no point of P maps to j.
 *   pcgc_offgrid_mse: out4 = (mean over p of best, max of best, mean over p of plane(p), max of plane) with plane(p) =
 *     mean_{q in T(p)} ((p - q) . normals_q)^2, the dot product as (dx*nx + dy*ny) + dz*nz; normals_q double [nq,3] or
 *     NULL: out4[2] = out4[3] = 0 then.  best double [np], plane double [np], n_ties int32 [np]: per point of P, all
 *     three or all NULL.
 * Deterministic (integer atomics / fixed-order double sums).  A Q that is not sorted or leaves the grid, or a coordinate
 * outside the stated limits (a NaN included), touches no memory out of bounds and gives NaN in every output. */
size_t pcgc_offgrid_workspace_bytes(int res, int64_t nq);
int pcgc_offgrid_transfer_normals(const float* p, int64_t np, const float* normals_p, const float* q, int64_t nq, double h,
                                  int ox, int oy, int oz, int res, double* normals_q, void* workspace,
                                  size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_offgrid_mse(const float* p, int64_t np, const float* q, int64_t nq, const double* normals_q, double h, int ox,
                     int oy, int oz, int res, double* out4, double* best, double* plane, int32_t* n_ties,
                     void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* Rigid registration (ICP) of a float32 source cloud P against a target Q: one step = correspondences under a trial pose,
 * reduced to the sums a point-to-point (Kabsch) or point-to-plane solve needs (pcgcv1_amd/register.py solves on the host;
 * DESIGN.md §7h; tests/_register_ref.py is the rule in numpy).  Q, its cells (h, ox, oy, oz, res) and the search are those
 * of pcgc_offgrid_* above; coordinates are in grid units (neighbouring surface points about 1 apart).
 *   pcgc_register_workspace_bytes: the off-grid workspace followed by 45 x 1024 doubles; 0 for a bad size.
 *   pcgc_register_prepare: the cells of Q (bit set, rank table, cell starts) into the workspace, once per target, and the
 *     flag cleared.  The workspace then belongs to that (q, nq, cells) until the next prepare.
 *   pcgc_register_step: R9 (row-major), t3, c3 are HOST doubles, taken by value.  All arithmetic is IEEE float64, one
 *     operation per step in the order written.  Per point i of P:
 *       p'   = float32(((R[3r] x + R[3r+1] y) + R[3r+2] z) + t[r]), r = 0, 1, 2, with x = double(P[i,0]) ...
 *       best = min over Q of d2(p', q), T = every j with |d2(p', q_j) - best| < 1e-8, w = 1.0 / double(|T|)
 *       used iff best <= max_dist * max_dist
 *     and per used point and j in T:  a = double(p') - c,  b = double(Q[j]) - c,  n = double(normals_q[j]) (float32
 *     [nq,3] in Q's order, taken as given, or NULL),
 *       res = ((a0-b0) n0 + (a1-b1) n1) + (a2-b2) n2
 *       J   = (a1 n2 - a2 n1, a2 n0 - a0 n2, a0 n1 - a1 n0, n0, n1, n2)
 *     out45 (double, device):
 *       [0]      number of used points (counted in integers)        [1]      sum of best, once per used point
 *       [2..4]   sum of w a_r            [5..7]   sum of w b_r       [8..16]  sum of (w a_r) b_c, row-major
 *       [17..37] sum of (w J_r) J_c for r <= c, the row-major upper triangle
 *       [38..43] sum of (w J_r) res      [44]     sum of (w res) res;       [17..44] are 0 when normals_q is NULL.
 *     The sums are float64 in a fixed order (per thread in grid-stride order, a fixed tree per workgroup, the workgroups
 *     in index order; no float atomics): the same input gives the same bits.  best double [np] and n_ties int32 [np]
 *     (0 for a point outside the gate) are optional, both or neither.
 *   A coordinate of p' that is a NaN or that no cell holds raises the step's flag in the workspace: out45 of that step is
 *   all NaN.  A Q that is not sorted or leaves the grid raises prepare's flag: every step is NaN until the next prepare.
 *   Neither touches memory out of bounds.  A step on a workspace that was not prepared for this (q, nq, cells) is
 *   undefined.  Rejects a null pointer, a max_dist that is not finite or <= 0, a pose or centre that is not finite, bad
 *   cells and a workspace smaller than pcgc_register_workspace_bytes. */
size_t pcgc_register_workspace_bytes(int res, int64_t nq);
int pcgc_register_prepare(const float* q, int64_t nq, double h, int ox, int oy, int oz, int res, void* workspace,
                          size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_register_step(const float* p, int64_t np, const float* q, int64_t nq, const float* normals_q, double h, int ox,
                       int oy, int oz, int res, const double* R9, const double* t3, const double* c3, double max_dist,
                       double* out45, double* best, int32_t* n_ties, void* workspace, size_t workspace_bytes,
                       pcgc_stream_t stream);

/* Global alignment: a start for the ICP above from any relative pose, by descriptor matching and RANSAC (pcgcv1_amd/
 * register.py draws and solves on the host; tests/_global_ref.py is the rule in numpy).  Four device stages,
 * every one with integer outputs that do not depend on the order of the work: the same input gives the same bytes, and
 * they equal numpy's.  The float64 arithmetic is IEEE, one operation per step in the order written.  Coordinates are in
 * grid units.  The keypoints K (float32 [n,3], n <= 2^24) are bucketed into the cells (h, ox, oy, oz, res) of pcgc_offgrid_*
 * above and passed SORTED ascending by cell key; normals float32 [n,3] in that order, unit or zero, taken as given.  A normal
 * is usable when its components are finite and not all zero.  d2 is that of pcgc_offgrid_*.
 *   N(i) = every j != i with 0 < d2(K_i, K_j) <= radius * radius and both normals usable; empty when normal i is not.
 *   pcgc_feature_pairs: per i and j in N(i), with d = double(K_i) - double(K_j), len = sqrt(d2), u = (dx/len, dy/len, dz/len),
 *       f1 = |(ni.x u.x + ni.y u.y) + ni.z u.z|,  f2 = the same with nj,  f3 = |(ni.x nj.x + ni.y nj.y) + ni.z nj.z|
 *       bin(f) = min(10, (int)floor(f * 11.0))
 *     S (uint32 [n,33]) = the counts of bin(f1) in [0,11), of bin(f2) in [11,22), of bin(f3) in [22,33); k (int32 [n]) = |N(i)|.
 *   pcgc_feature_combine: from S and k (as given), in uint64,
 *       G_i[b] = k_i S_i[b] + sum over N(i) of S_j[b],   T_i = k_i k_i + sum over N(i) of k_j
 *       feat_i[b] = (G_i[b] * 255 + T_i / 2) / T_i, integer division, 0 when T_i = 0 (at most 255 for S, k of pcgc_feature_pairs)
 *     feat uint8 [n,36] = the 33 bins and three zero bytes; valid uint8 [n] = (T_i > 0).
 *   Both build the cells in the workspace themselves.  radius must be positive and below 4 h.  Keypoints that are not
 *   sorted or leave the grid, or a NaN coordinate, touch no memory out of bounds and raise the workspace's flag: then k is
 *   -1 everywhere (pairs), valid 255 everywhere (combine).  The next call is not affected.
 *   pcgc_feature_match: rows uint8 [n,36] / [m,36], 4-byte aligned, and their valid bytes.  Per source row with a non-zero
 *     valid byte, over the target rows with one: dist (uint32) = the least sum over the 33 bins of (a - b)^2, j (int32) the
 *     lowest target row that reaches it.  j = -1 and dist = 0xFFFFFFFF for every other source row, and when no target row
 *     is valid.  The three bytes behind the bins are not read as data.  workspace: 8 n bytes, 8-byte aligned.
 *   pcgc_ransac_score: poses double [K,12] (device; R row-major, then t), P, Q float32 [C,3].  counts (int32 [K]) = the
 *     number of c with d2(p', Q_c) <= dist * dist, p' the moved point of pcgc_register_step, its float32 rounding included.
 *     A pose with a NaN counts none.
 *   All reject a null pointer, a size that is not positive or too large, bad cells, a radius or dist that is not finite
 *   and positive, and a workspace smaller than the sizer's figure (0 for a bad size), before any memory is touched. */
size_t pcgc_feature_workspace_bytes(int res, int64_t n);
int pcgc_feature_pairs(const float* keypoints, const float* normals, int64_t n, double h, int ox, int oy, int oz, int res,
                       double radius, uint32_t* S, int32_t* k, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_feature_combine(const float* keypoints, const float* normals, int64_t n, double h, int ox, int oy, int oz, int res,
                         double radius, const uint32_t* S, const int32_t* k, uint8_t* feat, uint8_t* valid, void* workspace,
                         size_t workspace_bytes, pcgc_stream_t stream);
size_t pcgc_feature_match_workspace_bytes(int64_t n);
int pcgc_feature_match(const uint8_t* source_rows, const uint8_t* source_valid, int64_t n, const uint8_t* target_rows,
                       const uint8_t* target_valid, int64_t m, int32_t* j, uint32_t* dist, void* workspace,
                       size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_ransac_score(const double* poses, int64_t n_poses, const float* P, const float* Q, int64_t C, double dist,
                      int32_t* counts, pcgc_stream_t stream);

/* Smoothing of a float cloud before it is voxelised: every point is projected onto the plane fitted to the points within
 * `radius` of it (pcgcv1_amd/smooth.py chains the passes; tests/_smooth_ref.py is the rule in numpy).  The
 * moments are exact integers and everything behind them is IEEE float64, one operation per step in the order written, so
 * nothing depends on the order of the points or of the threads: the same input gives the same bytes, and they equal numpy's.
 * points g (float32 [n,3], grid units) are bucketed into the cells (h, ox, oy, oz, res) of pcgc_offgrid_* above and passed
 * SORTED ascending by cell key; radius r within (0, 16] and r <= h, so a neighbourhood lies in a cell and its 26
 * neighbours; kmin within [3, 2^22].  d2 is that of pcgc_offgrid_*.
 *   N(i) = every j with d2(g_i, g_j) <= r * r: i itself and coincident points included.  K = |N(i)|.
 *   o_j  = llrint((double(g_j) - double(g_i)) * 65536.0) per component (sub, mul, round half to even), int64
 *   S = sum over N(i) of o_j (3 x int64);  Q = sum of o_j o_j^T (6 x int64: c00 c01 c02 c11 c12 c22, as pcgc_estimate_normals)
 *     |o| <= 2^20, so a term is below 2^41 and K <= 2^22 keeps every sum inside int64.
 *   K < kmin: out[i] = the bits of g_i, moved[i] = 0.  Otherwise moved[i] = 1 and
 *     m_a  = double(S_a) / double(K);   C_ab = double(Q_ab) / double(K) - m_a * m_b   (div, mul, sub)
 *     C goes through the cyclic Jacobi of pcgc_estimate_normals (at most 32 sweeps, rotations (0,1), (0,2), (1,2), the same
 *     thresholds); jx = the smallest diagonal entry by its selection a11 < a00 ? (a22 < a11 ? 2 : 1) : (a22 < a00 ? 2 : 0);
 *     n = that column of the eigenvector matrix divided by sqrt((n0*n0 + n1*n1) + n2*n2)
 *     t = (m_0 n_0 + m_1 n_1) + m_2 n_2;   d = t / 65536.0;   out[i,a] = float32(double(g[i,a]) + d * n_a)
 *   n needs no sign rule: negating it negates t exactly, and (-d)(-n_a) has the bits of d n_a.  C = 0 (every neighbour
 *   coincides with g_i) gives t = 0 and the input back (a coordinate -0.0 comes back as +0.0).
 *   out float32 [n,3] (not points itself: a pass reads the whole cloud and writes a new one), moved uint8 [n]; K int32 [n],
 *   S int64 [n,3], Q int64 [n,6] are optional debug outputs, all three or all NULL.
 *   Points that are not sorted or leave the grid, or a coordinate that is not finite, touch no memory out of bounds and
 *   raise the workspace's flag: moved is then 255 everywhere.  A point with more than 2^22 neighbours raises it too: moved
 *   is then 254 everywhere (the radius is too large for this density).  The other outputs of such a call mean nothing; the
 *   next call is not affected.  Rejects a null pointer, out == points, a size that is not positive or too large, bad cells, a
 *   radius outside (0, min(16, h)], a kmin outside [3, 2^22], one or two of K, S, Q, and a workspace smaller than
 *   pcgc_smooth_workspace_bytes (0 for a bad size), before any memory is touched. */
size_t pcgc_smooth_workspace_bytes(int res, int64_t n);
int pcgc_smooth_step(const float* points, int64_t n, double h, int ox, int oy, int oz, int res, double radius, int kmin,
                     float* out, uint8_t* moved, int32_t* K, int64_t* S, int64_t* Q, void* workspace,
                     size_t workspace_bytes, pcgc_stream_t stream);

/* Coloured ICP (Park, Zhou, Koltun 2017): a third registration metric that adds a photometric term to the point-to-plane
 * one, so that texture fixes the motions a plane, a sphere or a vase leaves free (pcgcv1_amd/register.py, metric="color";
 * DESIGN.md §7k; tests/_color_icp_ref.py is the rule in numpy).  Intensities are integers: Y = 2126 R + 7152 G + 722 B of a
 * uint8 colour (the BT.709 weights of pcgc_color_*), int32 within [0, 2550000], and I = double(Y) / 2550000.0.
 *
 * pcgc_color_gradient: per target point the least-squares gradient of I over the points within `radius`, constrained to the
 * point's tangent plane.  Built like pcgc_smooth_step: points g (float32 [n,3], grid units) in the cells (h, ox, oy, oz, res)
 * and SORTED ascending by cell key; normals float32 [n,3] and Y int32 [n] in that order; radius r within (0, 16] and r <= h;
 * kmin within [3, 2^20].  N(i), K and o_j are those of pcgc_smooth_step (d2 <= r * r, i itself included; o_j =
 * llrint((double(g_j) - double(g_i)) * 65536.0)).
 *   Q = sum over N(i) of o_j o_j^T (6 x int64: c00 c01 c02 c11 c12 c22);  B = sum of o_j (Y_j - Y_i) (3 x int64)
 *     |o| <= 2^20 and |Y_j - Y_i| < 2^22, so a term is below 2^42 and K <= 2^20 keeps every sum inside int64.
 *   g[i] = 0 and valid[i] = 0 when K < kmin, when a component of the normal is not finite or all three are zero, or when the
 *   determinant below is too small.  Otherwise valid[i] = 1 and, in IEEE float64, one operation per step in the order written,
 *   with n = double(normals[i]):
 *     k  = the axis of the smallest |n_k|, the first of equals:  |n1| < |n0| ? (|n2| < |n1| ? 2 : 1) : (|n2| < |n0| ? 2 : 0)
 *     c  = axis_k x n:  k = 0: (0.0, -n2, n1);  k = 1: (n2, 0.0, -n0);  k = 2: (-n1, n0, 0.0)
 *     e1 = c / sqrt((c0*c0 + c1*c1) + c2*c2) per component;   e2 = (n1 e1_2 - n2 e1_1, n2 e1_0 - n0 e1_2, n0 e1_1 - n1 e1_0)
 *     Qd_ab = double(Q_ab) / 4294967296.0;   Bd_a = (double(B_a) / 65536.0) / 2550000.0
 *     u = Qd e1, v = Qd e2, every row as (Qd_a0 e_0 + Qd_a1 e_1) + Qd_a2 e_2
 *     M00 = (e1_0 u0 + e1_1 u1) + e1_2 u2,  M01 = (e1_0 v0 + e1_1 v1) + e1_2 v2,  M11 = (e2_0 v0 + e2_1 v1) + e2_2 v2
 *     b0 = (e1_0 Bd_0 + e1_1 Bd_1) + e1_2 Bd_2,  b1 = the same with e2
 *     det = M00 * M11 - M01 * M01;  tr = M00 + M11;  too small iff !(det > 1e-6 * (tr * tr))   (collinear neighbours)
 *     x0 = (M11 * b0 - M01 * b1) / det;  x1 = (M00 * b1 - M01 * b0) / det;  g[i,a] = x0 * e1_a + x1 * e2_a
 *   g double [n,3], valid uint8 [n]; K int32 [n], Q int64 [n,6], B int64 [n,3] are optional debug outputs, all three or all
 *   NULL.  The same input gives the same bytes, and they equal numpy's.
 *   Points that are not sorted or leave the grid, a coordinate that is not finite or a Y outside [0, 2550000] touch no memory
 *   out of bounds and raise the workspace's flag: valid is then 255 everywhere.  A point with more than 2^20 neighbours raises
 *   it too: valid is then 254 everywhere (the radius is too large for this density).  The other outputs of such a call mean
 *   nothing; the next call is not affected.  Rejects a null pointer, a size that is not positive or too large, bad cells, a
 *   radius outside (0, min(16, h)], a kmin outside [3, 2^20], one or two of K, Q, B, and a workspace smaller than
 *   pcgc_color_gradient_workspace_bytes (0 for a bad size), before any memory is touched.
 *
 * pcgc_register_color_step: one ICP step of the colour metric.  p', best, T, w = 1 / |T| and the gate are exactly those of
 * pcgc_register_step, and so are the workspace's cells: pcgc_register_prepare fills a workspace of
 * pcgc_register_color_workspace_bytes (the off-grid workspace followed by 59 x 1024 doubles; 0 for a bad size) as it stands.
 * Yp int32 [np] goes with P; normals_q float32 [nq,3] (required), Yq int32 [nq], grad_q double [nq,3] and valid_q uint8 [nq]
 * (pcgc_color_gradient's g and valid) are in Q's order.  Per used point i and j in T, with a = double(p') - c,
 * b = double(Q[j]) - c, d = a - b per component, n = double(normals_q[j]), g = grad_q[j]:
 *     res = (d0 n0 + d1 n1) + d2 n2                            J  = (a1 n2 - a2 n1, a2 n0 - a0 n2, a0 n1 - a1 n0, n0, n1, n2)
 *   and only where valid_q[j] is not zero:
 *     rc  = (double(Yq[j]) / 2550000.0 - double(Yp[i]) / 2550000.0) + ((d0 g0 + d1 g1) + d2 g2)
 *     Jc  = (a1 g2 - a2 g1, a2 g0 - a0 g2, a0 g1 - a1 g0, g0, g1, g2)
 *   (g is orthogonal to n, so rc is the photometric residual of the paper with its projection onto the tangent plane folded in).
 *   out59 (double, device):
 *     [0]      number of used points (counted in integers)        [1]      sum of best, once per used point
 *     [2..22]  sum of (w J_r) J_c for r <= c, the row-major upper triangle
 *     [23..28] sum of (w J_r) res       [29]     sum of (w res) res
 *     [30]     sum of w over the pairs with a valid gradient
 *     [31..51] sum of (w Jc_r) Jc_c for r <= c                    [52..57] sum of (w Jc_r) rc       [58] sum of (w rc) rc
 *   The point-to-point moments of pcgc_register_step are left out.  The sums are float64 in the fixed order of
 *   pcgc_register_step: the same input gives the same bits.  best and n_ties are optional, both or neither.  Flags, what a
 *   flag does to the output (all NaN) and what is rejected are those of pcgc_register_step; every pointer but best and n_ties
 *   is required. */
size_t pcgc_color_gradient_workspace_bytes(int res, int64_t n);
int pcgc_color_gradient(const float* points, const float* normals, const int32_t* Y, int64_t n, double h, int ox, int oy, int oz,
                        int res, double radius, int kmin, double* g, uint8_t* valid, int32_t* K, int64_t* Q, int64_t* B,
                        void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
size_t pcgc_register_color_workspace_bytes(int res, int64_t nq);
int pcgc_register_color_step(const float* p, const int32_t* Yp, int64_t np, const float* q, const float* normals_q,
                             const int32_t* Yq, const double* grad_q, const uint8_t* valid_q, int64_t nq, double h, int ox, int oy,
                             int oz, int res, const double* R9, const double* t3, const double* c3, double max_dist, double* out59,
                             double* best, int32_t* n_ties, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* ---- Rendering (pcgcv1_amd/render.py; DESIGN.md "Rendering"; tests/_render_ref.py is the rule in numpy) ---------------
 * A cloud to an image: demo.ipynb:586,596,962,972 (o3d.visualization.draw_geometries), on a node without a display.
 * Orthographic, all integers after one rounding, so an image is defined bit for bit.
 *   points   float32 [n,3] (device), finite, |x| < 2^15; a point outside that (a NaN included) is dropped
 *   rotation int32 [9] (HOST), Q14, rows right, up, toward the viewer, entries within [-16384, 16384]
 *   window   u0, v1, w1 within (-2^31, 2^31); scale S within 1..2^30 = pixels per 1/16 voxel in Q16; |ox|, |oy| <= 2^20
 *   q   = (int) rintf(p * 16.0f) per coordinate, round half to even (1/16-voxel units)
 *   t_r = (rotation[3r] q0 + rotation[3r+1] q1 + rotation[3r+2] q2 + 8192) >> 14, r = 0, 1, 2, int64, arithmetic shift
 *   px  = (((t0 - u0) * S) >> 16) + ox,  py = (((v1 - t1) * S) >> 16) + oy,  d = w1 - t2  (a smaller d is nearer)
 * A point with d < 0 or d >= 2^31 is dropped.  Every other point i covers the point_size x point_size pixels centred on
 * (px, py), the part outside the image dropped, with key = (uint64(d) << 32) | i.
 *   pcgc_render_splat: workspace (uint64 [height, width], 8-byte aligned) = per pixel the smallest key of the points that
 *     cover it, all ones where none does: one 64-bit atomic min per covered pixel, skipped where the stored key is
 *     already smaller.  The minimum does not depend on arrival order; equal depths go to the lower index.  Rejects a
 *     null pointer (points may be NULL when n = 0), width or height outside 1..8192, point_size not odd or outside
 *     1..15, n outside [0, 2^32 - 1), a workspace smaller than pcgc_render_workspace_bytes (0 for a bad size).
 *   pcgc_render_resolve: rgb uint8 [height, width, 3]; index int32 [height, width] (the winner, -1 for background) and
 *     depth int32 [height, width] (its d, -1 for background) may be NULL.  An uncovered pixel takes `background`
 *     (0xRRGGBB).  A covered pixel with winner i takes c = colors[i] (uint8 [n,3], device), or `foreground` when colors
 *     is NULL or i >= n, shaded by eye-dome lighting of integer strength `shade` = k within 0..2^20 (0 = off):
 *       obs = sum over the eight neighbouring pixels inside the image and covered of max(0, d - d_neighbour)
 *       out = (c * ((255 k) / (k + obs)) + 127) / 255 per channel, integer divisions.
 *   pcgc_colormap: out[i] (uint8 [n,3]) = lut[min(255, (int) floorf(values[i] * scale))] with values float32 [n], finite
 *     and >= 0 (a NaN or a negative value takes entry 0), lut uint8 [256,3] (device), scale = float32(256 / vmax).
 * Deterministic (integer atomic min; everything else one thread per output). */
size_t pcgc_render_workspace_bytes(int width, int height);
int pcgc_render_splat(const float* points, int64_t n, const int32_t* rotation, int64_t u0, int64_t v1, int64_t w1, int32_t scale,
                      int32_t ox, int32_t oy, int width, int height, int point_size, void* workspace, size_t workspace_bytes,
                      pcgc_stream_t stream);
int pcgc_render_resolve(const void* workspace, size_t workspace_bytes, int width, int height, const uint8_t* colors, int64_t n,
                        uint32_t background, uint32_t foreground, int shade, uint8_t* rgb, int32_t* index, int32_t* depth,
                        pcgc_stream_t stream);
int pcgc_colormap(const float* values, int64_t n, float scale, const uint8_t* lut, uint8_t* out, pcgc_stream_t stream);

/* Recolouring: the colours of the original cloud S (int32 xyz < res, unique, uint8 rgb per point) carried onto the decoded
 * geometry T, passed like the D2 target as its linear keys (x*res + y)*res + z, int64, SORTED ascending and unique;
 * target_colors uint8 [n_t,3] and backward_counts int32 [n_t] (may be NULL) are in that order.  With N_T(s) = all points
 * of T at the minimal distance from s (ties kept) and B(t) = { s : t in N_T(s) }:
 *   colour(t) = per channel (2 sum_{s in B(t)} c_s + |B(t)|) / (2 |B(t)|), the mean rounded half up,
 *   over N_S(t), t's own nearest points of S, where B(t) is empty;  backward_counts[t] = |B(t)|.
 * Integer arithmetic throughout (32-bit atomic sums: n_s <= 2^32 / 255), so the result is defined bit for bit.
 * The workspace holds one occupancy bit set of res^3 cells and its rank table (popcount prefix per word). */
size_t pcgc_recolor_workspace_bytes(int res, int64_t n_s, int64_t n_t);
int pcgc_recolor(const int32_t* source_points, const uint8_t* source_colors, int64_t n_s, const int64_t* target_keys,
                 int64_t n_t, int res, uint8_t* target_colors, int32_t* backward_counts, void* workspace,
                 size_t workspace_bytes, pcgc_stream_t stream);

/* Colour distortion of MPEG pc_error 0.13.4 (`--color=1`), one direction: out3[i] = "c[i],    1" = mean over the points a
 * of A of (yuv_a[i] - yuv_m[i])^2, where m = per channel floor(mean of B's colours over ALL nearest points of B + 0.5)
 * in integers and yuv = BT.709 of rgb / 255 in float64 (Y = .2126 R + .7152 G + .0722 B, U = -.1146 R - .3854 G + .5 B + .5,
 * V = .5 R - .4542 G - .0458 B + .5).  Both clouds int32 xyz < res, unique, with uint8 rgb per point, in any order.  Call
 * twice (A->B, B->A); PSNR = -10 log10(mse), the symmetric figure takes the larger mse.  Deterministic (fixed-order sums). */
size_t pcgc_color_mse_workspace_bytes(int res, int64_t n_b);
int pcgc_color_mse(const int32_t* points_a, const uint8_t* colors_a, int64_t n_a, const int32_t* points_b,
                   const uint8_t* colors_b, int64_t n_b, int res, double* out3, void* workspace, size_t workspace_bytes,
                   pcgc_stream_t stream);

/* ---- RAHT colour transform (pcgcv1_amd/colorcodec.py; tests/_raht_ref.py is the rule in numpy) ----------
 * The region-adaptive hierarchical transform over the Morton order of M unique voxels with coordinates < 2^depth
 * (depth <= 12).  key = 3 depth bits, bit triple b from the top = x_b y_b z_b (pcgc_raht_keys; sort them with any sort).
 * Leaf j is the j-th key in ascending order.  The node that starts at leaf j > 0 is the right sibling of exactly one merge;
 * pcgc_raht_structure gives per leaf (device arrays, int32 [M]):
 *   subband[j] = the level l of that merge (the highest bit in which key[j] and key[j-1] differ); subband[0] = 3 depth (DC)
 *   left[j]    = the leaf at which its left sibling starts (weight w1 = j - left[j]);  w_right[j] = its own weight w2
 *   order[k]   = the leaves grouped by subband, ascending subband, ascending leaf within one (order[M-1] = 0)
 * and level_counts (HOST, int64 [3 depth + 1]) = leaves per subband; the call synchronises the stream once to read them.
 * It fails on keys that are not ascending, unique and below 2^(3 depth).
 *   pcgc_raht_forward / _inverse run in place on attr float64 [M,3] (leaf order): the merge of leaf j replaces
 *   (attr[left[j]], attr[j]) = (a1, a2) by (lo, hi) with lo = (sqrt(w1) a1 + sqrt(w2) a2) / sqrt(w1 + w2),
 *   hi = (sqrt(w1) a2 - sqrt(w2) a1) / sqrt(w1 + w2), levels ascending; the inverse undoes them, levels descending, with
 *   a1 = (sqrt(w1) lo - sqrt(w2) hi) / sqrt(w), a2 = (sqrt(w2) lo + sqrt(w1) hi) / sqrt(w).  After the forward pass attr[j]
 *   is the coefficient of subband[j] and attr[0] the DC.  One launch per level with merges; fuse_top != 0: every level
 *   from the first one above which at most 1024 leaves remain runs in ONE one-workgroup launch through LDS.  *launches
 *   (may be NULL) = kernel launches made.  Bit-exact float64 (no contraction, correctly rounded sqrt and division).
 *   pcgc_raht_load_colors: attr[j] = YCoCg-R (Co = R - B, t = B + (Co >> 1), Cg = G - t, Y = t + (Cg >> 1)) of the uint8 rgb of
 *   point point_of_leaf[j];  pcgc_raht_store_colors: rint, clip (Y [0,255], Co / Cg [-255,255]), inverse YCoCg-R, clip to
 *   [0,255], written to point point_of_leaf[j].
 *   pcgc_raht_quantize: q[k][c] = rint(coef[order[k]][c] / step) as int32 [M,3], and level_maxabs (device int32 [37],
 *   zeroed by the call) = max |q| per subband.  pcgc_raht_symbols: for k < n, symbol = q + amax[subband] where
 *   |q| <= amax[subband], else the escape symbol 2 amax + 1 (int16 [n,3]; amax device int32 [37], < 16383).
 *   pcgc_raht_dequantize: coef[order[k]][c] = (symbol - amax) * step for k < n (0 where escaped), then the patches
 *   patch int32 [n_patch,2] = (k * 3 + c, q) -> q * step (escaped values and the raw positions k >= n; everything else 0).
 * Workspace: max(37 int32 per 256 leaves + 512, 4 M) bytes, rounded up to 256 — about 4 M bytes; nothing per level. */
size_t pcgc_raht_workspace_bytes(int64_t m);
int pcgc_raht_keys(const int32_t* points, int64_t m, int64_t* keys, pcgc_stream_t stream);
int pcgc_raht_structure(const int64_t* sorted_keys, int64_t m, int depth, int32_t* subband, int32_t* left, int32_t* w_right,
                        int32_t* order, int64_t* level_counts, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_raht_forward(double* attr, int64_t m, int depth, const int32_t* left, const int32_t* w_right, const int32_t* subband,
                      const int32_t* order, const int64_t* level_counts, int fuse_top, int* launches, void* workspace,
                      size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_raht_inverse(double* attr, int64_t m, int depth, const int32_t* left, const int32_t* w_right, const int32_t* subband,
                      const int32_t* order, const int64_t* level_counts, int fuse_top, int* launches, void* workspace,
                      size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_raht_load_colors(const uint8_t* rgb, const int64_t* point_of_leaf, int64_t m, double* attr, pcgc_stream_t stream);
int pcgc_raht_store_colors(const double* attr, const int64_t* point_of_leaf, int64_t m, uint8_t* rgb, pcgc_stream_t stream);
int pcgc_raht_quantize(const double* coef, const int32_t* order, const int32_t* subband, int64_t m, double step, int32_t* q,
                       int32_t* level_maxabs, pcgc_stream_t stream);
int pcgc_raht_symbols(const int32_t* q, const int32_t* order, const int32_t* subband, int64_t n, const int32_t* amax,
                      int16_t* symbols, pcgc_stream_t stream);
int pcgc_raht_dequantize(const int16_t* symbols, int64_t n, const int32_t* patch, int64_t n_patch, const int32_t* order,
                         const int32_t* subband, const int32_t* amax, int64_t m, double step, double* coef,
                         pcgc_stream_t stream);
/* sums (device int64 [37 * 3], zeroed by the call): sums[subband * 3 + c] = sum over the rows k < n of q of subband `subband` of
 * min(|q[k][c]|, amax[subband] + 1) — the first moment colorcodec.choose_ratio fits a table to, so that the symbols need not
 * leave the device for a histogram.  amax as pcgc_raht_symbols takes it (after the per-level maxima are known). */
int pcgc_raht_abs_sums(const int32_t* q, const int32_t* order, const int32_t* subband, int64_t n, const int32_t* amax,
                       int64_t* sums, pcgc_stream_t stream);

/* ---- Colour rate control (csrc/color_rc.hip; colorcodec.encode_colors_target; tests/_color_rc_ref.py) ------
 * pcgc_raht_rate_sweep prices n_steps candidate steps (HOST double [n_steps], 1 <= n_steps <= 32, each positive and finite,
 * else -1 and nothing is launched) in one pass over coef (float64 [M,3] as pcgc_raht_forward leaves it): for the rows
 * k < k_raw of the subband order (the coded leaves) and q = rint(coef[order[k]][c] / steps[i]), pcgc_raht_quantize's expression,
 *   abs_sums (device int64 [n_steps][37][3]) [i][subband][c] = sum of min(|q|, 2048)  — what pcgc_raht_abs_sums gives after
 *   pcgc_raht_quantize at that step, since amax = min(max |q|, 2047);   max_abs (device int32 [n_steps][37]) [i][subband] =
 *   max |q|.  Both are zeroed by the call.  Integers only: exact, the same on every run.
 * pcgc_raht_requantize: out[j][c] = rint(coef[j][c] / step) * step for every row (quantise, then dequantise: escapes and the
 * raw tail carry q exactly); out must not overlap coef.
 * pcgc_color_sse6: two uint8 [M,3] colourings of the same points -> out (device int64 [6], zeroed by the call) = the sums of
 * dr^2, dg^2, db^2, dr dg, dr db, dg db with d = a - b: the squared error of any linear colour transform follows from them. */
int pcgc_raht_rate_sweep(const double* coef, const int32_t* order, const int32_t* subband, int64_t m, int64_t k_raw,
                         const double* steps, int n_steps, int64_t* abs_sums, int32_t* max_abs, pcgc_stream_t stream);
int pcgc_raht_requantize(const double* coef, int64_t m, double step, double* out, pcgc_stream_t stream);
int pcgc_color_sse6(const uint8_t* rgb_a, const uint8_t* rgb_b, int64_t m, int64_t* out, pcgc_stream_t stream);

/* ---- Chunked 64-way interleaved rANS, the entropy coder of colour stream version 2 (csrc/rans.hip; DESIGN.md 7d;
 * tests/_rans_ref.py is the rule in numpy) ---------------------------------------------------------------------------------
 * State uint32, lower bound 2^16, 16-bit words, 16-bit tables.  One wavefront per chunk; symbol j of a chunk belongs to lane
 * j % 64 and step j / 64.  All arrays are device arrays:
 *   symbols   int16 [n_symbols], as pcgc_raht_symbols writes them (flat [K,3]);
 *   chunks    int64 [n_chunks,3] = (level, index of the chunk's first symbol in `symbols`, n) with 1 <= n <= 64 steps_per_chunk;
 *             the table of symbol i is the level's table of channel i % 3;
 *   cdfs      int32 [cdf_total]: per level three tables of (symbols + 1) entries each, 0 .. 65536, every frequency >= 1;
 *             cdf_offsets int64 [n_levels + 1] = where each level's tables start; max_entries = the longest table (<= 4098).
 * pcgc_rans_encode writes the chunks' bytes (min(n, 64) final states as uint32, lane ascending, then the words in the order
 * the decoder takes them) back to back into out (2-byte aligned; 2 bytes per symbol of the chunks + 256 per chunk always suffice) and
 * offsets int64 [n_chunks + 1] = where each chunk starts, the last entry the total.  A chunk whose descriptor does not fit
 * the arrays is refused: it gets no bytes (offsets[c + 1] == offsets[c]).
 * pcgc_rans_decode reads payload (2-byte aligned) with the same offsets, writes the symbols and status int32 [n_chunks]:
 * 0 = ok, bit 0 = a final state differs from 2^16, bit 1 = words left over or missing, 4 = descriptor or byte range
 * refused (nothing of that chunk was read).  Every read of the stream is clamped to the chunk's own bytes. */
size_t pcgc_rans_workspace_bytes(int64_t n_chunks, int steps_per_chunk);
int pcgc_rans_encode(const int16_t* symbols, int64_t n_symbols, const int64_t* chunks, int64_t n_chunks, const int32_t* cdfs,
                     const int64_t* cdf_offsets, int n_levels, int64_t cdf_total, int max_entries, int steps_per_chunk, void* out,
                     int64_t out_bytes, int64_t* offsets, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_rans_decode(const void* payload, int64_t payload_bytes, const int64_t* offsets, const int64_t* chunks, int64_t n_chunks,
                     const int32_t* cdfs, const int64_t* cdf_offsets, int n_levels, int64_t cdf_total, int max_entries,
                     int steps_per_chunk, int16_t* symbols, int64_t n_symbols, int32_t* status, pcgc_stream_t stream);

/* points2voxels (dataprocess/inout_points.py:116-132) on device: scatter
 * n points (cube index, x, y, z as int32 x4) into zero-initialised float cubes. */
int pcgc_voxelize(const int32_t* cube_xyz, int64_t n, int cube_size, float* cubes,
                  int B, pcgc_stream_t stream);
/* The same straight from pcgc_partition's outputs (process.py:33-36 runs partition and points2voxels back to back):
 * points int32 [n,3] global coordinates, cube_of_point int32 [n] index into the key-sorted cubes (-1 = point of a
 * dropped cube); fills the zero-initialised cubes [cube_hi - cube_lo, cs, cs, cs] of the cubes cube_lo <= c < cube_hi
 * (a rank's block; 0, B for all).  Coordinates are reduced mod cube_size here. */
int pcgc_voxelize_points(const int32_t* points, const int32_t* cube_of_point, int64_t n, int cube_size,
                         int cube_lo, int cube_hi, float* cubes, pcgc_stream_t stream);

/* ---- encoder-side point counts (.pointnums) for the smallest cube-local D1 ----------------------------------------
 * The decoder keeps, per cube, the voxels whose logit is >= the k-th largest, ties included, with k = the stored count
 * (select_voxels / get_adaptive_thres, dataprocess/inout_points.py:147-179; pcgc_topk_threshold).  eval's rho search
 * (eval_ablation_studies.py:152-205) picks one rho for the whole cloud with the original at hand; these entry points let
 * the encoder pick every cube's k instead.  cubes: x float32 [B, cs, cs, cs] (occupied: x > 0), logits the same shape,
 * both on the device; cs <= 256.  Coordinates are the voxel indices inside the cube; distances squared, in integers.
 *
 * pcgc_pointnums_count: k_max int32 [B] (1 <= k_max <= cs^3) -> thresholds[b] = the k_max-th largest logit,
 * n_pts[b] = #occupied voxels, n_seg[b] = #voxels with logit >= thresholds[b] (all device).
 *
 * pcgc_pointnums_curves: for cubes whose counts came from pcgc_pointnums_count, with device int64 offsets pts_off /
 * seg_off / curve_off [B+1] (prefix sums of n_pts, n_seg and k_max, starting at 0; total_seg / total_pts their last
 * entries) and block lists seg_blocks / pts_blocks (int32 pairs (cube, first element) cutting every cube's n_seg /
 * n_pts elements into pieces of 256): for k = 1 .. k_max[b], at curve_off[b] + k - 1,
 *   m = |S(k)|, S(k) = { v : logit[v] >= the k-th largest logit }  (-0.0 == +0.0),
 *   A = sum over occupied p of min over v in S(k) |p - v|^2,   B = sum over v in S(k) of min over occupied p |v - p|^2
 * (B = 0 for a cube without occupied voxels).  Exact integers; the memory of one call grows with total_seg: call it on
 * chunks of cubes (pcgcv1_amd/pointnums.py).
 *
 * pcgc_pointnums_sweep: the curves above -> for assignment a < J + 1 and every cube, k_out[a B + b] = argmin over k of
 * a A(k) + (J - a) B(k) in int64 (ties: the smallest k); for a = J + 1 + l, k_out = fixed_k[l B + b] clamped to
 * 1 .. k_max[b].  sums[3 a + {0, 1, 2}] = sum over the cubes of A, B, m at the assignment's k (device int64). */
int pcgc_pointnums_count(const float* x, const float* logits, const int32_t* k_max, int B, int cube_size,
                         float* thresholds, int32_t* n_pts, int32_t* n_seg, pcgc_stream_t stream);
size_t pcgc_pointnums_curves_workspace_bytes(int64_t total_seg, int64_t total_pts);
int pcgc_pointnums_curves(const float* x, const float* logits, const float* thresholds, int B, int cube_size,
                          const int64_t* pts_off, const int64_t* seg_off, const int64_t* curve_off, int64_t total_seg,
                          int64_t total_pts, const int32_t* seg_blocks, int n_seg_blocks, const int32_t* pts_blocks,
                          int n_pts_blocks, int32_t* m, int64_t* A, int64_t* Bc, void* workspace,
                          size_t workspace_bytes, pcgc_stream_t stream);
size_t pcgc_pointnums_sweep_workspace_bytes(int B, int n_assign);
int pcgc_pointnums_sweep(const int32_t* m, const int64_t* A, const int64_t* Bc, const int64_t* curve_off, int B, int J,
                         const int32_t* fixed_k, int L, int32_t* k_out, int64_t* sums, void* workspace,
                         size_t workspace_bytes, pcgc_stream_t stream);

/* ---- the same for the smallest cube-local D2 (point-to-plane) ----
 * Stands in for eval's rho_d2 search (eval_ablation_studies.py:152-205 with the RHOS_D2 ladder of line 196; the figure is
 * pc_error's "mseF,PSNR (p2plane)", myutils/pc_error_wrapper.py:46-51), which picks one rho per cloud at the decoder's side.
 *
 * pcgc_pointnums_normals: point_key int64 [n_points] = cube * cs^3 + voxel index of every input point under the mapping of
 * pcgc_voxelize_points (< 0: a point of a dropped cube), normals float32 [n_points, 3], vox_key int64 [n_vox] the distinct
 * keys >= 0 in ascending order (= the occupied voxels, cube by cube, in ascending voxel index: the P order of
 * pcgc_pointnums_curves) -> vox_normals int16 [n_vox, 4] = (nx, ny, nz, 0), the normal of the voxel's lowest-index point as
 * rint(1024 n / |n|) (float64, half to even); a zero or non-finite normal gives (0, 0, 0).  All on the device.
 *
 * pcgc_pointnums_curves_d2: pcgc_pointnums_curves with vox_normals int16 [total_pts, 4] of the call's cubes (8-byte
 * aligned).  m as there; with v*(p, k) the voxel of S(k) nearest to p (ties: the lowest rank under logit descending, index
 * ascending) and p*(v) the occupied voxel nearest to v (ties: the smallest voxel index),
 *   A2 = sum over occupied p of ((v* - p) . n_q(p))^2,   B2 = sum over v in S(k) of ((p* - v) . n_q(p*))^2
 * in the same flat layout, so pcgc_pointnums_sweep serves as it is.  One term is at most 3 (cs - 1)^2 1026^2: the caller
 * cuts chunks so that (total_pts + total_seg) times that stays below 2^62. */
size_t pcgc_pointnums_normals_workspace_bytes(int64_t n_vox);
int pcgc_pointnums_normals(const int64_t* point_key, const float* normals, int64_t n_points, const int64_t* vox_key,
                           int64_t n_vox, int16_t* vox_normals, void* workspace, size_t workspace_bytes,
                           pcgc_stream_t stream);
size_t pcgc_pointnums_curves_d2_workspace_bytes(int64_t total_seg, int64_t total_pts);
int pcgc_pointnums_curves_d2(const float* x, const float* logits, const float* thresholds, const int16_t* vox_normals, int B,
                             int cube_size, const int64_t* pts_off, const int64_t* seg_off, const int64_t* curve_off,
                             int64_t total_seg, int64_t total_pts, const int32_t* seg_blocks, int n_seg_blocks,
                             const int32_t* pts_blocks, int n_pts_blocks, int32_t* m, int64_t* A2, int64_t* B2,
                             void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* ---- mesh -> point cloud with normals (dataprocess/mesh2pc_open3d.py:55-85) ---- */
/* sample_points_uniformly + np.dot(points, get_rotate_matrix()) (mesh2pc_open3d.py:57-66).  vertices double [V,3],
 * triangles int32 [T,3], area_cdf double [T] = inclusive running sum of the triangle areas (pcgc_mesh_area_cdf), all on
 * the device; points double [n_points,3].  rotation: a row-major 3x3 double matrix on the device, or NULL for none.
 * Sample i draws u_k = (h_k >> 11) * 2^-53, k = 0, 1, 2, where h_k is the (3i + k + 1)-th output of splitmix64 seeded
 * with `seed`:  z = seed + (3i + k + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 * z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  h = z ^ (z >> 31)  (all mod 2^64).
 * Triangle t = upper_bound(area_cdf, u0 * area_cdf[T-1]) (zero-area triangles are never chosen; a target that rounds
 * up to the total takes the last triangle of positive area).  s = sqrt(u1), a = 1 - s, b = s (1 - u2), c = s u2,
 * p = (a v0 + b v1) + c v2 per coordinate; rotated as a row vector: p'_k = (p_x m_0k + p_y m_1k) + p_z m_2k.
 * Every step is one IEEE double operation in this order, without contraction. */
int pcgc_mesh_sample(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                     const double* area_cdf, int64_t n_points, uint64_t seed, const double* rotation, double* points,
                     pcgc_stream_t stream);
/* The voxelisation of mesh2pc_open3d.py:67-73 + np.unique(points, axis=0): m = min over all 3n coordinates,
 * M = max of p - m, q = rint((p - m) / M * resolution) (half to even; M == 0 gives 0), then the distinct q in
 * lexicographic order, int32 [n_out,3].  cap >= n (the output never holds more than n rows); *n_out (DEVICE int64)
 * receives the count.  1 <= resolution <= 4095; workspace holds a (resolution+1)^3 bit set. */
size_t pcgc_mesh_voxelize_workspace_bytes(int resolution);
int pcgc_mesh_voxelize(const double* points, int64_t n, int resolution, int32_t* out, int64_t cap, int64_t* n_out,
                       void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
/* estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) (mesh2pc_open3d.py:75-78) on a voxel grid.
 * points int32 [n,3], any order, 0 <= coordinate < res <= 4096; radius <= 16, 1 <= max_nn <= 64; normals float32 [n,3]
 * in input order (duplicate points share a cell and its normal).
 *   neighbours: the first max_nn occupied cells of the offset table = every integer offset d with |d|^2 <= radius^2
 *     ("<=": whether Open3D's radius test is inclusive could not be checked), sorted by (|d|^2, dx, dy, dz); offset 0,
 *     the point itself, counts.  K = their number.
 *   C = K sum d d^T - (sum d)(sum d)^T, exact in int64 (d = the offsets, not the absolute coordinates).
 *   normal: the eigenvector of the smallest eigenvalue of C (cyclic Jacobi in double); K < 3: (0,0,1); C of rank <= 1
 *     (every 2x2 minor 0: collinear neighbours): u = the row of C with the largest diagonal entry (lowest index on
 *     ties), j = the axis of u's smallest |component| (lowest index on ties), normal = normalize(u x e_j).
 *   sign: flipped so that the first component with |c| > 1e-6 is positive (Open3D leaves it arbitrary).
 * cov int64 [n,6] (c00 c01 c02 c11 c12 c22) and n_neighbours int32 [n]: optional debug outputs (both or neither).
 * pcgc_normals_table_size: the number of offsets within `radius` (4169 at radius 10), -1 for a bad radius. */
int pcgc_normals_table_size(double radius);
size_t pcgc_normals_workspace_bytes(int res, int64_t n, double radius);
int pcgc_estimate_normals(const int32_t* points, int64_t n, int res, double radius, int max_nn, float* normals, int64_t* cov,
                          int32_t* n_neighbours, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* ---- raw scan -> voxel cloud with colours and normals (pcgcv1_amd/ingest.py; tests/_ingest_ref.py is
 * the rule in numpy) ----
 * A scan has float coordinates in its own units and any number of points per voxel.  A frame (origin[3], step, bits),
 * 1 <= bits <= 12, puts it on the grid of res = 2^bits cells per axis, R = res - 1.  All position arithmetic is IEEE
 * float64, one operation per step in the stated order, without contraction.
 *   pcgc_ingest_bounds: out[0..2] = per-axis minimum, out[3..5] = per-axis maximum over the rows of points (double
 *     [n,3], device) whose three coordinates are all finite; *n_dropped (DEVICE int64) = the number of the other rows.
 *     When every row is dropped out = (+inf x 3, -inf x 3).  out: DEVICE double [6].  n >= 1.
 *   pcgc_ingest_quantize: q_k = floor((p_k - origin_k) / step + 0.5) as sub, div, add, floor, then clamped to [0, R];
 *     q int32 [n,3], keys int64 [n] = (q_x * res + q_y) * res + q_z.  A row with a non-finite coordinate gets q = -1,
 *     -1, -1 and key -1.  origin: HOST double [3], finite; step finite and > 0.
 *   pcgc_ingest_merge: one row per occupied voxel in ascending key (np.unique's order).  keys int64 [n]: a key outside
 *     [0, res^3) contributes nothing.  colors uint8 [n,3] or NULL, normals float32 [n,3] or NULL (then the matching
 *     output may be NULL too).  Per voxel:
 *       out_points  int32 [cap,3]: the cell of the key;   out_counts int32 [cap]: its number of input rows;
 *       out_colors  uint8 [cap,3]: (2 sum + count) / (2 count) in integers per channel: the exact mean, half rounded up;
 *       out_normals float32 [cap,3]: each input component c -> double, non-finite -> 0, clamped to [-1, 1], then the int64
 *         rint(c * 2^30) (half to even); v = the three int64 sums as double, len = sqrt((vx*vx + vy*vy) + vz*vz); the
 *         output is float(v / len), or (0, 0, 0) when len == 0.
 *     Everything summed is an integer (int32 / uint32 / int64 atomics), so no output depends on the order of the rows or
 *     of the threads.  *n_out (DEVICE int64) = the number of rows; rows at and beyond cap are not written: cap >=
 *     min(n, res^3) holds them all.  The colour sums are uint32: with colours n <= 16 843 009 (2^32 / 255), which no
 *     voxel's sum can overflow.  1 <= n < 2^31.  workspace: pcgc_ingest_workspace_bytes(bits, n) (0 for a bad argument),
 *     a bit set and a rank table over res^3 cells and the accumulators of n voxels. */
int pcgc_ingest_bounds(const double* points, int64_t n, double* out, int64_t* n_dropped, pcgc_stream_t stream);
int pcgc_ingest_quantize(const double* points, int64_t n, const double* origin, double step, int bits, int32_t* q,
                         int64_t* keys, pcgc_stream_t stream);
size_t pcgc_ingest_workspace_bytes(int bits, int64_t n);
int pcgc_ingest_merge(const int64_t* keys, int64_t n, int bits, const uint8_t* colors, const float* normals,
                      int32_t* out_points, int32_t* out_counts, uint8_t* out_colors, float* out_normals, int64_t cap,
                      int64_t* n_out, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* ---- outlier voxels of a scan: neighbourhood statistics (pcgcv1_amd/clean.py; tests/_clean_ref.py is the
 * rule in numpy) ----
 * points int32 [n,3], distinct, on the grid of res = 2^bits cells per axis, 1 <= bits <= 12; 0 <= k <= 64; 1 <= radius
 * R <= 32.  For a voxel p, N(p) = the multiset of squared distances d2(p, q) over the occupied q != p with d2 <= R * R (a
 * Euclidean ball).  isqrt16(d) = floor(sqrt(d * 2^32)), from an exact integer table over d = 0 .. 1024.
 *   cnt int32 [n]: |N(p)|;
 *   S   int64 [n]: the sum of isqrt16 over the min(k, cnt) smallest members of N(p), plus (k - min(k, cnt)) * ((R + 1) <<
 *     16): a neighbour the ball does not hold is charged as if it sat at distance R + 1.  Ties at the k-th distance do
 *     not matter (equal distances, equal terms).
 * All integer, independent of the order of the rows and of the threads; a ball that leaves the grid is clipped to it.  S
 * or cnt may be NULL, not both; with k == 0, S must be NULL.  A point outside the grid sets no bit, is nobody's neighbour
 * and gets S = k * ((R + 1) << 16), cnt = 0.  A bad argument returns an error before any memory is touched.  1 <= n <
 * 2^31.  workspace: pcgc_clean_workspace_bytes(bits, n) (0 for a bad argument), the bit set over res^3 cells. */
size_t pcgc_clean_workspace_bytes(int bits, int64_t n);
int pcgc_clean_neighbors(const int32_t* points, int64_t n, int bits, int k, int radius, int64_t* S, int32_t* cnt,
                         void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* ---- islands of a scan: connected components (pcgcv1_amd/clean.py; tests/_components_ref.py is the rule in
 * numpy) ----
 * points int32 [n,3], distinct, on the grid of res = 2^bits cells per axis, 1 <= bits <= 12; the gap G, 1 <= G <= 8.  Two
 * voxels p != q are linked when max(|dx|, |dy|, |dz|) <= G (G = 1: 26-connectivity); the window is clipped to the grid and
 * nothing wraps from the end of a row, a plane or the grid into the next.  The components are the classes of the transitive
 * closure of the link.
 *   label int64 [n]: the smallest linear key (x * res + y) * res + z over p's component, so ascending labels follow
 *     np.unique's order;
 *   size  int32 [n]: the number of voxels of p's component (may be NULL);
 *   n_components int64 [1]: the number of distinct labels (may be NULL).
 * All integer, independent of the order of the rows and of the threads; two calls give the same bytes.  A point outside
 * the grid sets no bit, belongs to no component, is not counted and gets label = -1, size = 0.  A bad argument returns an
 * error before any memory is touched.  1 <= n < 2^31.  The number of launches is fixed and nothing is read back.
 * workspace: pcgc_clean_components_workspace_bytes(bits, n) (0 for a bad argument): the bit set and its rank table over
 * res^3 cells, then 16 bytes per point. */
size_t pcgc_clean_components_workspace_bytes(int bits, int64_t n);
int pcgc_clean_components(const int32_t* points, int64_t n, int bits, int gap, int64_t* label, int32_t* size,
                          int64_t* n_components, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* ---- the floor or table of a scan: plane scoring and selection (pcgcv1_amd/clean.py; tests/_plane_ref.py is
 * the rule in numpy) ----
 * points int32 [n,3] on the grid of res = 2^bits cells per axis, 1 <= bits <= 12.  A plane is five int64 numbers (a, b, c,
 * d, T); a voxel (x, y, z) is an inlier when |a x + b y + c z - d| <= T in exact integers.  T < 0 matches nothing, and a
 * point with a coordinate outside the grid is never an inlier.  The caller makes the planes (clean.draw_planes,
 * clean.refit_plane): for a normal (a, b, c) through p0 and a distance of D2 half cells, d = (a, b, c) . p0 and T =
 * isqrt(D2^2 (a^2 + b^2 + c^2)) / 2, which is exactly 2 |s| <= D2 |(a, b, c)|.
 *   pcgc_plane_count: planes int64 [K,5], 1 <= K <= 65536 -> counts int32 [K], the number of inliers of every plane.  Meant
 *     for draws, the cross products of three voxels: |a|, |b|, |c| < 2^26, T < 2^31, |s| < 2^40 at 12 bits; a plane whose
 *     a, b, c do not fit int32 is counted through 64-bit products, chosen per plane on the device.
 *   pcgc_plane_select: plane int64 [5] -> mask uint8 [n], 1 = inlier, and sums int64 [10] (may be NULL) over the inliers: N,
 *     sum x, sum y, sum z, sum x^2, sum y^2, sum z^2, sum xy, sum xz, sum yz.  Meant for any plane up to the refit's:
 *     |a|, |b|, |c| < 2^47, T < 2^54, |s| < 2^62.
 * The arithmetic is modulo 2^64: beyond those bounds a count or a mask is unspecified and nothing out of bounds is touched.
 * All integer, independent of the order of the rows and of the threads; two calls give the same bytes.  counts and sums are
 * zeroed by the call itself.  A bad argument (a null pointer other than sums, n outside 1 .. 2^31 - 1, K outside 1 ..
 * 65536, bits outside 1 .. 12) returns an error before any memory is touched.  No workspace, a fixed number of launches and
 * nothing is read back. */
int pcgc_plane_count(const int32_t* points, int64_t n, int bits, const int64_t* planes, int64_t K, int32_t* counts,
                     pcgc_stream_t stream);
int pcgc_plane_select(const int32_t* points, int64_t n, int bits, const int64_t* plane, uint8_t* mask, int64_t* sums,
                      pcgc_stream_t stream);

/* ---- a triangle mesh from a voxel cloud (pcgcv1_amd/surface.py; tests/_surface_ref.py is the rule in numpy) ----
 * points int32 [n,3], distinct, on the grid of res = 2^bits cells per axis, 1 <= bits <= 12, 1 <= n < 2^31; normals float32
 * [n,3] of unit length.  All float arithmetic is float64 in the order written here, without contraction.
 *
 * Orientation (pcgc_surface_orient): sign int8 [n] in {+1, -1} such that sign * normal is consistent over a component.  Two
 * voxels are linked as in pcgc_clean_components with the gap G, 1 <= G <= 8.  seed uint8 [n] marks one voxel per component
 * (the caller picks the one with the largest key); its sign is -1 if nx < 0 else +1.  Rounds are Jacobi: a round reads the signs
 * the round before left.  With the stage thresholds tau[0 .. n_tau) (1 <= n_tau <= 8, each within [0, 1], the last 0.0) and the
 * stage k, 0 at the start, a round takes for every unset voxel i, among its linked voxels j that are set, the j with the
 * largest |c_ij|, c_ij = (nix njx + niy njy) + niz njz, the smallest key among equals, and if |c_ij| >= tau[k] sets sign[i] =
 * sign[j] * (+1 if c_ij >= 0 else -1).  A round that set something puts k back to 0, one that set nothing raises it by one;
 * rounds run while a voxel is unset.  *rounds (host) = the number of rounds run, *readbacks (host, may be NULL) = the number of
 * times the 16-byte state was read back: `batch` rounds (1..4096) are queued per read, which changes neither sign nor rounds.
 * The call synchronises the stream.  A component without a seed is an error (sign is not written).
 *
 * The lattice (pcgc_surface_lattice): a cell is the unit box centred on an integer point c; the candidate cells are the voxels
 * and their 26 neighbours, unclipped, c in [-1, res]^3.  Lattice vertex k stands at k + 0.5; the corners of cell c are
 * c - 1 + {0,1}^3, so k lies in [-2, res]^3, and its key is ((kx + 2) * S + (ky + 2)) * S + (kz + 2) with S = res + 3.  counts
 * int64 [2] (device) = the number of candidate cells and of their distinct corners.  The workspace keeps both sets for the
 * calls below, which must follow with the same bits, n and workspace.
 *
 * The implicit value (pcgc_surface_implicit): oriented_normals float64 [n,3] = sign * normal, radius R in 3..8; n_vertices =
 * counts[1].  vertex_keys int64 [n_vertices] ascending; f float64 [n_vertices]: over the occupied q = k + o, o in [-R, R+1]^3
 * ascending in (ox, oy, oz), with dd = (2k + 1) - 2q and d2 = |dd|^2 (integers), skipping d2 > 4 R^2: t = 1.0 - d2 / (4 R^2 + 1),
 * w = t * t, num += w * ((Nx ddx + Ny ddy) + Nz ddz), W += w; f = 0.5 * num / W.  A vertex is inside iff f < 0.  Every vertex
 * sees a voxel within 1.5 sqrt 3 < R, so W > 0.
 *
 * Marching tetrahedra (pcgc_surface_triangles, twice: with `count` int64 [1] (device) and triangle_ids NULL it counts, with
 * triangle_ids int64 [n_triangles,3] and count NULL it writes).  Every candidate cell with lowest corner v0 is cut into the six
 * Kuhn tetrahedra (v0, v0 + e_p0, v0 + e_p0 + e_p1, v0 + (1,1,1)), one per permutation p of the axes in lexicographic order.  A
 * lattice edge whose ends a < b differ in `inside` carries a mesh vertex with the id key(a) * 7 + direction, the directions
 * b - a = 100 010 001 110 101 011 111 numbered 0..6.  With I and O the inside and outside corners in the tetrahedron's order:
 * one inside corner gives (I0 O0, I0 O1, I0 O2), three give (I0 O0, I1 O0, I2 O0), two give the quad I0 O0, I0 O1, I1 O1, I1 O0
 * as (1st, 2nd, 3rd) and (1st, 3rd, 4th).  A triangle keeps that order when sign(p) * sign of the sequence (I.., O..) as a
 * permutation of 0..3 is positive and has its last two corners swapped otherwise: counter-clockwise seen from f >= 0, decided
 * without a float test, so zero-area triangles (an f of exactly 0) are wound like their neighbours and kept.  Triangles come in
 * the order of the cells' keys.
 *
 * The mesh (pcgc_surface_mesh): edge_ids int64 [n_edges] = the distinct triangle_ids ascending (the caller sorts); vertices
 * float64 [n_edges,3]: with t = f_a / (f_a - f_b), a + 0.5 + t (b - a) per axis as (a + 0.5) + t * (b - a); triangles int32
 * [n_triangles,3] = the index of each id in edge_ids.
 *
 * Integer atomics only: two calls give the same bytes.  A bad argument returns an error before any memory is touched.  Only
 * pcgc_surface_orient reads anything back.  Rows that repeat or leave the grid are the caller's to refuse; they index nothing out
 * of bounds.  workspace: pcgc_surface_workspace_bytes(bits, n) (0 for a bad argument): bit sets and rank tables over res^3 and
 * (res + 3)^3 cells, a bit set over (res + 2)^3, and 30 bytes per point. */
size_t pcgc_surface_workspace_bytes(int bits, int64_t n);
int pcgc_surface_orient(const int32_t* points, const float* normals, const uint8_t* seed, int64_t n, int bits, int gap,
                        const double* tau, int n_tau, int batch, int8_t* sign, int32_t* rounds, int32_t* readbacks,
                        void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_surface_lattice(const int32_t* points, int64_t n, int bits, int64_t* counts, void* workspace,
                         size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_surface_implicit(const double* oriented_normals, int64_t n, int bits, int radius, int64_t n_vertices,
                          int64_t* vertex_keys, double* f, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_surface_triangles(const double* f, int64_t n_vertices, int64_t n, int bits, int64_t n_triangles,
                           int64_t* triangle_ids, int64_t* count, void* workspace, size_t workspace_bytes,
                           pcgc_stream_t stream);
int pcgc_surface_mesh(const int64_t* edge_ids, int64_t n_edges, const int64_t* triangle_ids, int64_t n_triangles,
                      const double* f, int64_t n_vertices, int64_t n, int bits, double* vertices, int32_t* triangles,
                      void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* ---- a smaller mesh: quadric vertex clustering (pcgcv1_amd/surface.py: simplify; tests/_simplify_ref.py is the
 * rule in numpy) ----
 * vertices float64 [V,3] in voxel units, finite and within [-2, res + 2) on every axis, res = 2^bits, 1 <= bits <= 12, 1 <= V <
 * 2^31; triangles int32 [T,3] with indices in 0..V-1, 3 T < 2^31; cell an integer in 1..64.  All float arithmetic is float64 in
 * the order written here, without contraction; the sums start at 0.0.
 *
 * 0. Canonical order (the caller's): every triangle rotated so that its smallest index comes first, the rows sorted
 *    lexicographically.  Everything below takes the triangles in that order, so the result is a function of the mesh as a set of
 *    oriented triangles.
 * 1. Clusters (pcgc_simplify_keys): c = floor((v + 2.0) / cell) per axis, M = (res + 4 + cell - 1) / cell (integers), the key
 *    (cx * M + cy) * M + cz; -1 for a vertex outside the range.  The clusters are the distinct keys ascending (the caller
 *    uniques), K of them; rank int32 [V] = the position of a vertex' key among them.  A cluster's centre is o = (c + 0.5) * cell -
 *    2.
 * 2. Quadric.  A triangle belongs to each of the distinct clusters of its three corners, once each; a cluster takes its triangles
 *    in ascending canonical position.  pcgc_simplify_incidence writes words int32 [T,3]: the rank of each corner, or K where an
 *    earlier corner of the same triangle has that rank already; the caller sorts the 3 T words stably, tri_entry int64 [3 T] =
 *    the indices of the sorted words (entry e is corner e % 3 of triangle e / 3), tri_start int64 [K + 1] = where each rank's run
 *    starts (tri_start[K] = the first word K); vert_index int64 [V] = the vertices sorted stably by rank and vert_start int64
 *    [K + 1] likewise.  Per triangle with the corners v0 v1 v2: q0 = v0 - o, e1 = (v1 - o) - q0, e2 = (v2 - o) - q0, n = e1 x e2 as
 *    (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x) (unnormalised: the weight is the squared area), d = -((nx q0x + ny
 *    q0y) + nz q0z); A += (nx nx, nx ny, nx nz, ny ny, ny nz, nz nz), b += (nx d, ny d, nz d).  sum += v - o over the cluster's
 *    vertices in ascending index, m = sum / count.
 * 3. Placement (pcgc_simplify_place): r_i = (-b_i) - ((A_i0 m0 + A_i1 m1) + A_i2 m2); the cyclic Jacobi of the normal estimation
 *    (csrc/jacobi3.h) on a copy of A gives the eigenvalues l_i and the eigenvectors E_i (columns); lmax = the largest l_i; s = 0,
 *    and for i = 0, 1, 2 with l_i > 1e-3 * lmax: t = ((E_0i r0 + E_1i r1) + E_2i r2) / l_i, s_j = s_j + E_ji * t; x = m + s.  Where
 *    lmax is not positive or some |x_j| > cell / 2 (the optimum left the cube) the cluster falls back to x = m and fallback uint8
 *    [K] is 1.  placed float64 [K,3] = o + x.  The truncation keeps a flat or a creased cluster well-posed.
 * 4. Triangles, as a chain (pcgc_simplify_remap, then the caller's sort, unique and integer scatter-add).  Every corner maps to
 *    its rank; a triangle with two equal corners is degenerate: triples int32 [T,3] = (-1, -1, -1), sign int32 [T] = 0, packed -1.
 *    Otherwise, rotated so that its smallest rank a comes first, it reads (a, b, c): triples = (a, lo, hi) = (a, min(b, c),
 *    max(b, c)), sign = +1 if b < c else -1, packed int64 [T] (may be NULL; needs K <= 2^21) = a << 42 | lo << 21 | hi.  The net
 *    multiplicity of a triple is the sum of the signs of the triangles that map to it: 0, the triple vanishes (cancelled);
 *    otherwise it gives one triangle, (a, lo, hi) if positive and (a, hi, lo) if negative (folded where the absolute value is 2 or
 *    more).  The output triangles ascend in (a, lo, hi); the clusters none of them names are removed and the rest renumbered in
 *    ascending key.  The output is the image of the input 2-chain under the vertex map: where no triple is folded, a closed input
 *    gives an output in which every undirected edge is traversed equally often in both directions.
 *
 * No atomics, no workspace, nothing read back; two calls give the same bytes.  A bad argument returns an error before any memory
 * is touched.  Vertices outside the range and indices outside the vertices are the caller's to refuse; every index is checked
 * before it is used, so they touch nothing out of bounds. */
int pcgc_simplify_keys(const double* vertices, int64_t n_vertices, int bits, int cell, int64_t* keys, pcgc_stream_t stream);
int pcgc_simplify_incidence(const int32_t* triangles, int64_t n_triangles, const int32_t* rank, int64_t n_vertices,
                            int64_t n_clusters, int32_t* words, pcgc_stream_t stream);
int pcgc_simplify_place(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                        const int64_t* cluster_keys, int64_t n_clusters, int bits, int cell, const int64_t* tri_start,
                        const int64_t* tri_entry, const int64_t* vert_start, const int64_t* vert_index, double* placed,
                        uint8_t* fallback, pcgc_stream_t stream);
int pcgc_simplify_remap(const int32_t* triangles, int64_t n_triangles, const int32_t* rank, int64_t n_vertices,
                        int64_t n_clusters, int32_t* triples, int32_t* sign, int64_t* packed, pcgc_stream_t stream);

/* ---- a mesh against its cloud: the distance from a point to a triangle mesh (pcgcv1_amd/metrics.py: mesh_error; DESIGN.md §7n;
 * tests/_mesh_error_ref.py is the rule in numpy, by brute force) ----
 * points float64 [N,3], vertices float64 [V,3], triangles int32 [T,3] with indices in 0..V-1; every coordinate finite with
 * |coordinate| < 2^20; 1 <= N, V < 2^31, 1 <= T, 3 T < 2^31.  Everything is IEEE float64, each operation one step in the order
 * written, without contraction.  For three-vectors x and y:
 *   x - y   = (x0 - y0, x1 - y1, x2 - y2)
 *   x . y   = (x0 * y0 + x1 * y1) + x2 * y2
 *   x cross y = (x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0)
 *   min of x and y = x < y ? x : y
 * The rule, for a point p and a triangle (a, b, c) (csrc/point_triangle.h is this text as code, for the host and the device):
 *   seg of p, u, v:  e = v - u, w = p - u, l = e . e, s = w . e;  t = 0 when !(l > 0), otherwise t = s / l, then t = 0 if t < 0,
 *                then t = 1 if t > 1;  r_k = w_k - t * e_k;  the value is r . r.
 *   face:        n = (b - a) cross (c - a), nn = n . n;  u = a - p, v = b - p, w = c - p.  The face term counts iff nn > 0 and
 *                n . (u cross v) >= 0 and n . (v cross w) >= 0 and n . (w cross u) >= 0.  Its value is dn * dn / nn (the product
 *                first) with dn = n . (p - a).
 *   d2 of p and the triangle:  m = min of (seg of p, a, b) and (seg of p, b, c);  m = min of m and (seg of p, c, a);  where the face term
 *                counts, m = min of m and the face term.
 * A triangle of zero area is a segment or a point; nothing divides by zero.
 * Per point: best = the minimum of d2 over all triangles, nearest = the smallest triangle index that attains it.  With a gate
 * max_dist (> 0; +infinity for none) a point with best > max_dist * max_dist is far: best = +infinity, nearest = -1.  The
 * figures: out4[0] = the sum of best over the points that are not far, in the caller's point order (per thread in grid-stride
 * order over 256 * min(ceil(N / 256), 1024) threads, a fixed tree per workgroup, the workgroups in index order), divided by
 * their number; out4[1] = the maximum of those best; both NaN where every point is far; out4[2] = the number of far points;
 * out4[3] = the number of point-triangle pairs evaluated (the one figure that depends on the cells).  best, nearest and the
 * other figures depend on the points and the triangle list alone: not on the cells, not on `order`.
 *
 * The search lists every triangle in each cubic cell of edge h (a power of two >= 1) that its axis-aligned bounding box
 * overlaps; the cell of a coordinate x is floor(x / h) - origin, inside a grid of res^3 cells, res <= 1024, that holds the whole
 * mesh:
 *   pcgc_meshdist_count: counts int64 [T] = the cells each triangle's box overlaps.  The caller scans them.
 *   pcgc_meshdist_emit:  words int64 [n_pairs] (n_pairs = the sum, < 2^31): for triangle t, from offsets[t] (the exclusive scan)
 *                on, cell key << 31 | t for the cells of its box in x, y, z order, key = (x * res + y) * res + z.  The caller sorts
 *                the words ascending: by cell and, inside a cell, by triangle.
 *   pcgc_meshdist_prepare: from the sorted words, the cells in the workspace (bit set, rank table, starts: csrc/voxel_grid.h,
 *                csrc/offgrid_cells.h) and packed float64 [T,9] = the corners of every triangle side by side.
 *   pcgc_meshdist_query: the walk of one thread per point over Chebyshev shells of cells about its own (which may lie outside
 *                the grid), clipped to the grid.  After the shell of half-width w every triangle not met lies farther than w h
 *                from p, so the walk ends once min(best, max_dist^2) < (1 - 2^-20) (w h)^2, or with the grid; the margin covers
 *                the rounding of d2 (csrc/point_triangle.h argues it).  order int32 [N] (or NULL): a permutation; thread s takes
 *                point order[s], so a caller that sorts the points by cell has the lanes of a wave walk the same cells.  best
 *                float64 [N] and nearest int32 [N] are written at the caller's index.
 * flag int32 [1], zeroed by the caller before the first call, is raised by a triangle that names a vertex outside 0..V-1, a
 * coordinate that is not finite or reaches 2^20, a triangle outside the grid, offsets or words that do not fit, an order entry
 * outside 0..N-1.  The query then returns NaN in out4 and in every best, and -1 in every nearest.  Every index is checked
 * before it is used, so none of this touches memory out of bounds.  No float atomics: two calls give the same bytes. */
int pcgc_meshdist_count(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double h, int ox,
                        int oy, int oz, int res, int64_t* counts, int32_t* flag, pcgc_stream_t stream);
int pcgc_meshdist_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double h, int ox,
                       int oy, int oz, int res, const int64_t* offsets, int64_t n_pairs, int64_t* words, int32_t* flag,
                       pcgc_stream_t stream);
size_t pcgc_meshdist_workspace_bytes(int res, int64_t n_pairs, int64_t n_points);
int pcgc_meshdist_prepare(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                          const int64_t* words, int64_t n_pairs, int res, int64_t n_points, double* packed, int32_t* flag,
                          void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_meshdist_query(const double* points, int64_t n_points, const int32_t* order, const double* packed, int64_t n_triangles,
                        int64_t n_pairs, double h, int ox, int oy, int oz, int res, double max_dist, double* out4, double* best,
                        int32_t* nearest, int32_t* flag, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);

/* ---- training step (train_hyper.py:174-214) ------------------------------ */
/* Gradient of one Conv3D / Conv3DTranspose layer.  D = spatial size of the layer's INPUT x; dz = gradient w.r.t.
 * the layer's pre-activation output (apply pcgc_relu_bwd first), contiguous [B,Do^3,Cout].  Replaces what
 * tf.GradientTape derives for tf.keras.layers.Conv3D/Conv3DTranspose (train_hyper.py:202-207).
 * bwd_data: dx [B,D^3,Cin];  bwd_weight: dkernel in the layer's TF layout, dbias [Cout] or NULL.
 * Deterministic (two-stage fixed-order reductions).  workspace: pcgc_conv3d_bwd_workspace_bytes. */
size_t pcgc_conv3d_bwd_workspace_bytes(int Cin, int Cout, int ksize);
int pcgc_conv3d_bwd_data(const float* dz, const float* kernel, float* dx, int B, int D, int Cin, int Cout,
                         int ksize, int stride, int transposed, void* workspace, size_t workspace_bytes,
                         pcgc_stream_t stream);
/* bwd_data with the elementwise neighbours of the reverse pass fused into its epilogue:
 *   dx = (relu_mask > 0) ? (add_to + conv_bwd_data(dz)) : 0
 * relu_mask (or NULL) = the layer's forward input x when x is a ReLU output — the gradient of the producing ReLU, so the
 * caller needs no pcgc_relu_bwd for it; add_to (or NULL, may alias dx) = gradient already accumulated for x from its
 * other consumers (the residual branch of a VRN block).  Both [B,D^3,Cin] like dx. */
int pcgc_conv3d_bwd_data_fused(const float* dz, const float* kernel, float* dx, const float* relu_mask,
                               const float* add_to, int B, int D, int Cin, int Cout, int ksize, int stride,
                               int transposed, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
int pcgc_conv3d_bwd_weight(const float* x, const float* dz, float* dkernel, float* dbias, int B, int D,
                           int Cin, int Cout, int ksize, int stride, int transposed, void* workspace,
                           size_t workspace_bytes, pcgc_stream_t stream);
/* dz[v,c] = dy[v*dy_cs + dy_co + c] * (y[v,c] > 0)  (ReLU backward on a channel slice of dy; y NULL = copy). */
int pcgc_relu_bwd(const float* dy, int dy_cs, int dy_co, const float* y, float* dz, int64_t nvox, int C,
                  pcgc_stream_t stream);
/* out = relu(x + concat(t12, t23))  — the block tail of _VoxceptionResNet.call (model_voxception.py:65-67); C = channels
 * of x, a multiple of 8. */
int pcgc_vrn_merge(const float* x, const float* t12, const float* t23, float* out, int64_t nvox, int C,
                   pcgc_stream_t stream);
int pcgc_add_inplace(float* a, const float* b, int64_t n, pcgc_stream_t stream);
/* Reverse of the block tail out = relu(x + concat(t12, t23)) in one pass (model_voxception.py:65-67 differentiated):
 *   dpre = dout * (out > 0)            (premasked != 0: dout already carries that mask, dpre is not written and may be NULL)
 *   dz12 = dpre[:, :C/2] * (t12 > 0),  dz23 = dpre[:, C/2:] * (t23 > 0)     — the gradients w.r.t. the pre-activation
 * outputs of conv1_2 / conv2_3, what pcgc_conv3d_bwd_* take.  C = channels of out. */
int pcgc_vrn_bwd_split(const float* dout, const float* out, const float* t12, const float* t23, float* dpre, float* dz12,
                       float* dz23, int64_t nvox, int C, int premasked, pcgc_stream_t stream);
/* t23 == NULL: t12 is the concatenated [nvox, C] tensor (`pre` of pcgc_vrn_fwd_train). */
/* The same pair for blocks whose forward kept only the SIGNS of the pre-residual output: pre_signs int32 [B,D,D,D],
 * bit c = (pre[c] > 0) — all the reverse pass reads of `pre` (2 B of information per voxel instead of 64 B written and
 * read back).  For C = 16 the word also carries the other ReLU masks of the block's reverse: bits 16-19 = (t22 > 0),
 * 20-23 = (t11 > 0), 24-27 = (t21 > 0); pcgc_vrn_bwd_tail_split takes them from there and does not read t11 / t21 / t22
 * (their pointers must still be valid tensors; PCGC_DEBUG_SIGNS=1 makes the entry points compare the bits with the tensors first
 * and refuse words that do not carry the masks).  pcgc_vrn_fwd_train_signs: as pcgc_vrn_fwd_train, where pcgc_vrn_fwd_train_signs_supported(D, C) != 0
 * (D = 64 with C = 16, D = 32 with C = 32); pcgc_vrn_bwd_split_signs: as pcgc_vrn_bwd_split with the masks (t12 > 0), (t23 > 0) taken from
 * the bits (C <= 32). */
int pcgc_vrn_fwd_train_signs_supported(int D, int C);
int pcgc_vrn_fwd_train_signs(const float* x, const float* const* params, float* t11, float* t21, float* t22,
                             int32_t* pre_signs, float* out, int B, int D, int C, pcgc_stream_t stream);
int pcgc_vrn_bwd_split_signs(const float* dout, const float* out, const int32_t* pre_signs, float* dpre, float* dz12,
                             float* dz23, int64_t nvox, int C, int premasked, pcgc_stream_t stream);
/* The Q4 layout of the training step's 64^3 stage.  The C = 16 blocks' row kernels read a voxel row as one VGPR per
 * channel; on NDHWC tensors that is 16 B per lane at a 64 B stride, on Q4 [b][d][h][C/4][w][4] one contiguous KiB per
 * wave instruction (the inference path's layout).  With Trainer(q4=True) the 16-channel tensors of the stage (conv_in's
 * output ... down_1's input, up_2's output ... deconv_out's input, and their gradients) and the blocks' 8-channel
 * gradients are Q4; 4-channel tensors are the same in both layouts.  pcgc_vrn_fwd_train_q4 / pcgc_vrn_bwd_tail_split_q4 /
 * pcgc_vrn_bwd_input_q4 are the _signs / _split / _input entry points on such tensors; the boundary layers and the
 * weight gradients learn the layout per layer through pcgc_train_plan_set_layout.  pcgc_layout_q4 converts
 * (tests, tools): to_q4 = 1 NDHWC -> Q4, 0 back; C a multiple of 4. */
int pcgc_vrn_fwd_train_q4(const float* x, const float* const* params, float* t11, float* t21, float* t22,
                          int32_t* pre_signs, float* out, int B, int D, int C, pcgc_stream_t stream);
int pcgc_layout_q4(const float* src, float* dst, int B, int D, int C, int to_q4, pcgc_stream_t stream);

/* Reverse of the block's inner convolutions in one pass (model_voxception.py:59-60, 62-64 differentiated), from the
 * outputs of pcgc_vrn_bwd_split(_signs):
 *   dt11 = [t11 > 0] * conv1_2^T(dz12),   dt22 = [t22 > 0] * conv2_3^T(dz23),   dt21 = [t21 > 0] * conv2_2^T(dt22)
 * dz12 / dz23 [B,D,D,D,C/2]; t11 / t21 / t22 (the forward's saved ReLU outputs) and dt11 / dt21 / dt22 [B,D,D,D,C/4];
 * kernel12 [3,3,3,C/4,C/2], kernel22 [3,3,3,C/4,C/4], kernel23 [1,1,1,C/4,C/2] in the TensorFlow layouts.  dt11 / dt21
 * feed pcgc_vrn_bwd_input; the three layers' dW stay with pcgc_train_conv_bwd_weight (x = t11 / t21 / t22,
 * dz = dz12 / dt22 / dz23).  Only where pcgc_vrn_bwd_tail_supported(D, C) != 0 (D = 64 with C = 16). */
int pcgc_vrn_bwd_tail_supported(int D, int C);
int pcgc_vrn_bwd_tail(const float* dz12, const float* dz23, const float* t11, const float* t21, const float* t22,
                      const float* kernel12, const float* kernel22, const float* kernel23, float* dt11, float* dt21,
                      float* dt22, int B, int D, int C, pcgc_stream_t stream);

/* pcgc_vrn_bwd_split_signs (premasked form) and pcgc_vrn_bwd_tail in ONE pass: dout [B,D,D,D,C] already carries the mask
 * (out > 0); dz12 / dz23 are made from it and the sign bits for every row the kernel touches and written once (the
 * weight gradients of conv1_2 / conv2_3 read them), dt11 / dt21 / dt22 as above.  pcgc_vrn_bwd_tail_split_supported:
 * D = 64 with C = 16 (other blocks: pcgc_vrn_bwd_split_signs, then pcgc_vrn_bwd_tail). */
int pcgc_vrn_bwd_tail_split_supported(int D, int C);
int pcgc_vrn_bwd_tail_split(const float* dout, const int32_t* pre_signs, const float* t11, const float* t21,
                            const float* t22, const float* kernel12, const float* kernel22, const float* kernel23,
                            float* dz12, float* dz23, float* dt11, float* dt21, float* dt22, int B, int D, int C,
                            pcgc_stream_t stream);
int pcgc_vrn_bwd_tail_split_q4(const float* dout, const int32_t* pre_signs, const float* t11, const float* t21,
                               const float* t22, const float* kernel12, const float* kernel22, const float* kernel23,
                               float* dz12, float* dz23, float* dt11, float* dt21, float* dt22, int B, int D, int C,
                               pcgc_stream_t stream);                       /* dout, dz12, dz23 Q4 */

/* Reverse of the block head in one pass: the three contributions to the gradient of the block input
 * (x feeds conv1_1, conv2_1 and the skip connection, model_voxception.py:57-58, 61, 65-67):
 *   dx = [x > 0] * ( dpre + conv1_1^T(dt11) + conv2_1^T(dt21) )
 * dt11 / dt21 [B,D,D,D,C/4]: gradients w.r.t. the pre-activation outputs of conv1_1 / conv2_1; dpre / dx [B,D,D,D,C]
 * (dx may alias dpre); x_mask = the block input where it is a ReLU output, NULL for no mask; kernel11 / kernel21 in the
 * TensorFlow layouts [3,3,3,C,C/4] / [1,1,1,C,C/4].  The dW of the two layers stay with pcgc_train_conv_bwd_weight.
 * Only where pcgc_vrn_bwd_input_supported(D, C) != 0 (D = 64 with C = 16). */
int pcgc_vrn_bwd_input_supported(int D, int C);
int pcgc_vrn_bwd_input(const float* dt11, const float* dt21, const float* dpre, const float* x_mask, const float* kernel11,
                       const float* kernel21, float* dx, int B, int D, int C, pcgc_stream_t stream);
int pcgc_vrn_bwd_input_q4(const float* dt11, const float* dt21, const float* dpre, const float* x_mask, const float* kernel11,
                          const float* kernel21, float* dx, int B, int D, int C, pcgc_stream_t stream);   /* dpre / x_mask / dx Q4 */

/* Forward of one _VoxceptionResNet block for the training step (train_hyper.py:184-196 runs the same
 * model_voxception.py:56-68 call under the tape): pcgc_vrn_fwd's row kernels on NDHWC tensors, keeping what the reverse
 * pass reads — t11 = relu(conv1_1(x)), t21 = relu(conv2_1(x)), t22 = relu(conv2_2(t21)) [B,D,D,D,C/4] each, and
 * pre = concat[relu(conv1_2(t11)), relu(conv2_3(t22))] [B,D,D,D,C] (out = relu(x + pre)).  Only where
 * pcgc_vrn_fwd_train_supported(D, C) != 0 (D = 64 with C = 16, D = 32 with C = 32); other blocks run layer by layer. */
int pcgc_vrn_fwd_train_supported(int D, int C);
int pcgc_vrn_fwd_train(const float* x, const float* const* params, float* t11, float* t21, float* t22, float* pre,
                       float* out, int B, int D, int C, pcgc_stream_t stream);

/* ---- training plan: the step's per-layer housekeeping batched (csrc/train_plan.hip) ----
 * One entry per Conv3D / Conv3DTranspose of the trained sub-models (train_hyper.py:202-214: the variables the tape
 * differentiates and the optimiser updates).  kernel / dkernel / dbias point into the caller's parameter and gradient
 * buffers and must stay valid and in place for the plan's lifetime; dbias NULL = layer without bias. */
typedef struct pcgc_train_layer {
  const float* kernel;
  float* dkernel;
  float* dbias;
  int Cin, Cout, ksize, stride, transposed;
} pcgc_train_layer;
typedef struct pcgc_train_plan pcgc_train_plan;
int pcgc_train_plan_create(const pcgc_train_layer* layers, int n_layers, pcgc_train_plan** out);
void pcgc_train_plan_destroy(pcgc_train_plan* plan);
int pcgc_train_plan_layers(const pcgc_train_plan* plan);
/* Once per step, after the optimiser update and before the forward pass: packs / flips every filter from the current
 * parameter values (two launches for all layers) and resets the pool of weight-gradient partial sums. */
int pcgc_train_plan_prepare(pcgc_train_plan* plan, pcgc_stream_t stream);
/* pcgc_conv3d_fwd / pcgc_conv3d_bwd_data_fused / pcgc_conv3d_bwd_weight of layer `layer` on the prepared filters;
 * D = spatial size of the layer's input.  Results are bit-identical to those entry points.  bwd_weight only produces
 * partial sums: dkernel / dbias of every layer are written by pcgc_train_plan_finish_weights (one launch per 56
 * pending reductions), to be called once after the last bwd_weight of the step. */
/* x_q4 / y_q4 != 0: this layer's input / output tensor (and the gradients laid out like them) are Q4 in every later
 * call on the layer (see pcgc_vrn_fwd_train_q4); shapes without a kernel for that fail with an error, never silently. */
int pcgc_train_plan_set_layout(pcgc_train_plan* plan, int layer, int x_q4, int y_q4);
int pcgc_train_conv_fwd(const pcgc_train_plan* plan, int layer, const float* x, const float* bias, float* y, int B, int D,
                        int relu, pcgc_stream_t stream);
int pcgc_train_conv_bwd_data(const pcgc_train_plan* plan, int layer, const float* dz, float* dx, const float* relu_mask,
                             const float* add_to, int B, int D, pcgc_stream_t stream);
int pcgc_train_conv_bwd_weight(pcgc_train_plan* plan, int layer, const float* x, const float* dz, int B, int D,
                               pcgc_stream_t stream);
/* Two independent stride-1 layers of a VRN block (model_voxception.py:56-66) in ONE launch where a pair kernel exists — the
 * 16^3 blocks of a training batch, whose layers alone are 512 workgroups of 11-37 us: conv1_1 | conv2_1 (xa == xb),
 * conv1_2 | conv2_2, and in reverse conv1_2^T | conv2_3^T (dx_i = (relu_mask_i > 0) * conv_i^T(dz_i), nothing accumulated).
 * Every other pair of shapes runs as exactly the two single calls above; results are bit-identical either way. */
int pcgc_train_conv_fwd_pair(const pcgc_train_plan* plan, int layer_a, int layer_b, const float* xa, const float* xb,
                             const float* bias_a, const float* bias_b, float* ya, float* yb, int B, int D, int relu_a, int relu_b,
                             pcgc_stream_t stream);
int pcgc_train_conv_bwd_data_pair(const pcgc_train_plan* plan, int layer_a, int layer_b, const float* dz_a, const float* dz_b,
                                  float* dx_a, float* dx_b, const float* relu_mask_a, const float* relu_mask_b, int B, int D,
                                  pcgc_stream_t stream);
/* Two layers in one launch where the second needs from the first only what the same workgroup wrote (16^3 blocks again):
 *  _bwd_data_chain: the reverse of the block's two input layers (layer_b 1x1x1), dx = m * (m * (dx + conv_a^T(dz_a)) + conv_b^T(dz_b))
 *                   in place on dx (the gradient the skip connection brought), m = (relu_mask > 0), or 1 when relu_mask is NULL;
 *  _fwd_merge:      conv2_3 (1x1x1, y = tensor2_3) and the block's merge out = relu(blk_x + concat(t12, y)) (pcgc_vrn_merge).
 * Other shapes run as the single calls; bit-identical either way (the same sums in the same order). */
int pcgc_train_conv_bwd_data_chain(const pcgc_train_plan* plan, int layer_a, int layer_b, const float* dz_a, const float* dz_b,
                                   float* dx, const float* relu_mask, int B, int D, pcgc_stream_t stream);
int pcgc_train_conv_fwd_merge(const pcgc_train_plan* plan, int layer, const float* x, const float* bias, float* y, int relu,
                              const float* blk_x, const float* t12, float* out, int C, int B, int D, pcgc_stream_t stream);
/* conv1_1 (3x3x3) and conv2_1 (1x1x1) of a VRN block (model_voxception.py:56-62) read the same tensor: both layers'
 * partial sums in one pass over x where the fused kernel exists (16 | Cin, Cout 4 or 8), else exactly the two calls above.
 * The 3x3x3 layer's sums are those of pcgc_train_conv_bwd_weight bit for bit; the 1x1x1 layer's are added in another
 * (fixed) order. */
int pcgc_train_conv_bwd_weight_pair(pcgc_train_plan* plan, int layer3, int layer1, const float* x, const float* dz3,
                                    const float* dz1, int B, int D, pcgc_stream_t stream);
int pcgc_train_plan_finish_weights(pcgc_train_plan* plan, pcgc_stream_t stream);
/* on != 0 (off by default): the weight gradients of the stride-1 layers at D <= 16 — the 16^3 stage and the hyperprior nets
 * of the train_hyper step (train_hyper.py:200-207), ~35 launches of 128-512 workgroups per step — are recorded by
 * pcgc_train_conv_bwd_weight and launched by pcgc_train_plan_finish_weights, equal shapes as the jobs of ONE launch.  The
 * caller must then keep x and dz of such calls alive and unchanged until pcgc_train_plan_finish_weights.  Same kernels and
 * sums per layer: the gradients are bit-identical.  Switch it between steps only. */
int pcgc_train_plan_defer_small(pcgc_train_plan* plan, int on);
/* dscale == NULL: out = max(|s_raw|, lower_bound) (model_voxception.py:308 + train_hyper.py:189);
 * else out = dscale * sign(s_raw) * (|s_raw| >= lower_bound)  (its gradient, TF conventions). */
int pcgc_abs_max(const float* s_raw, float lower_bound, const float* dscale, float* out, int64_t n,
                 pcgc_stream_t stream);
/* Gradients of coef * sum(log(max(likelihood, bound))) w.r.t. the (noisy) values, loc and scale
 * (conditional_entropy_model.py:34-56 differentiated; sign() has zero gradient). */
int pcgc_laplace_likelihood_bwd(const float* values, const float* loc, const float* scale, float coef,
                                float likelihood_bound, float* dvalues, float* dloc, float* dscale, int64_t n,
                                pcgc_stream_t stream);
/* Same for the factorized prior (entropy_model.py:72-98, 114-151): dvalues [n] and dparams in the packed
 * tensor order of pcgc_factorized_likelihood.  C must divide 256. */
size_t pcgc_factorized_bwd_workspace_bytes(int C);
int pcgc_factorized_likelihood_bwd(const float* values, const float* params, float coef, float likelihood_bound,
                                   float* dvalues, float* dparams, int64_t n, int C, void* workspace,
                                   size_t workspace_bytes, pcgc_stream_t stream);
/* d/dpred of w0 * mean_{label=0}(-log(1-o)) + w1 * mean_{label>0}(-log o) (loss.py:8-33); pass w0/n0, w1/n1. */
int pcgc_bce_bwd(const float* pred, const float* label, float w0_over_n0, float w1_over_n1, float* dpred,
                 int64_t n, pcgc_stream_t stream);
/* The three reverse kernels above with their coefficients formed ON THE DEVICE from counts that are still there: the
 * reference divides the loss terms by the number of occupied / empty voxels (train_hyper.py:193-199), which the step only
 * knows after its forward pass — a host that reads them back stalls the stream in the middle of the step.
 *   pcgc_bce_bwd_dev:            w0/n0 = (float)(a0 / sums4[1]), w1/n1 = (float)(a1 / sums4[3]), sums4 = pcgc_bce_sums' output;
 *   pcgc_*_likelihood_bwd_dev:   coef = (float)(num / (mul * *count))   (e.g. num = delta, mul = -ln 2, count = &sums4[3]).
 * The same double-precision expressions the host forms: identical gradients. */
int pcgc_bce_bwd_dev(const float* pred, const float* label, const double* sums4, double a0, double a1, float* dpred,
                     int64_t n, pcgc_stream_t stream);
int pcgc_laplace_likelihood_bwd_dev(const float* values, const float* loc, const float* scale, double num, double mul,
                                    const double* count, float likelihood_bound, float* dvalues, float* dloc,
                                    float* dscale, int64_t n, pcgc_stream_t stream);
int pcgc_factorized_likelihood_bwd_dev(const float* values, const float* params, double num, double mul,
                                       const double* count, float likelihood_bound, float* dvalues, float* dparams,
                                       int64_t n, int C, void* workspace, size_t workspace_bytes, pcgc_stream_t stream);
/* out = sum(log(p)) in double, fixed order (train_hyper.py:194-196). */
size_t pcgc_sum_log_workspace_bytes(void);
int pcgc_sum_log(const float* p, int64_t n, double* out, void* workspace, size_t workspace_bytes,
                 pcgc_stream_t stream);
/* The training step's three loss reductions in two launches (train_hyper.py:193-199: the BCE sums of the logits against
 * the occupancy, sum log(likelihood) of y and of z): sums4 as pcgc_bce_sums, logs2 = {pcgc_sum_log(lik_y), pcgc_sum_log(lik_z)},
 * bit-identical to the three separate calls (the same blocks run the same sums). */
size_t pcgc_train_loss_sums_workspace_bytes(int64_t n);
int pcgc_train_loss_sums(const float* pred, const float* label, int64_t n, const float* lik_y, int64_t n_y,
                         const float* lik_z, int64_t n_z, double* sums4, double* logs2, void* workspace,
                         size_t workspace_bytes, pcgc_stream_t stream);
/* tf.train.AdamOptimizer update (TF1 form, train_hyper.py:104, 209-214); lr_t = lr*sqrt(1-b2^t)/(1-b1^t). */
int pcgc_adam_step(float* param, const float* grad, float* m, float* v, int64_t n, float lr_t, float beta1,
                   float beta2, float epsilon, pcgc_stream_t stream);
/* The same update, skipped ON THE DEVICE when the step's BCE sums (sums4 of pcgc_train_loss_sums, still on the device) say the
 * batch had no empty or no occupied voxel (sums4[1] == 0 or sums4[3] == 0: loss.py:8-33 divides by both counts, the gradients
 * are inf / NaN).  Lets the host queue the update before it reads the loss terms back instead of idling the GPU for the
 * read-back; the host still raises on such a batch, with the parameters untouched. */
int pcgc_adam_step_guarded(float* param, const float* grad, float* m, float* v, int64_t n, float lr_t, float beta1,
                           float beta2, float epsilon, const double* bce_sums4, pcgc_stream_t stream);

/* ------------------------------------------------------------------ */
/* libpcgc_host.so — sequential host tail (no HIP dependency)          */
/* ------------------------------------------------------------------ */
const char* pcgc_host_last_error(void);

/* coder_ops.pmf_to_quantized_cdf (entropy_model.py:218). pmf [rows,n] -> cdf int32 [rows,n+1]. */
int pcgc_pmf_to_quantized_cdf(const float* pmf, int64_t rows, int n, int precision, int32_t* cdf);
/* coder_ops.range_encode (entropy_model.py:258; conditional_entropy_model.py:161).
 * data int16 [rows, cols]; cdf int32 [(rows|1)*cols, n+1] (broadcast_rows=1 for the
 * [1,C,N+1] table).  Writes up to cap bytes, returns the length in *out_len (if it
 * exceeds cap the function returns -2 and the caller retries with a bigger buffer). */
int pcgc_range_encode(const int16_t* data, int64_t rows, int cols, const int32_t* cdf, int n,
                      int broadcast_rows, int precision, uint8_t* out, int64_t cap, int64_t* out_len);
/* The same stream from the rounded VALUES: symbol = data[i] - offset (data int8 or int16, elem_bytes 1 or 2) — the z string
 * of entropy_model.py:249-259 without a pass over the batch to subtract min_v first (millions of symbols for a large cloud,
 * on the one thread everything else then waits for). */
int pcgc_range_encode_values(const void* data, int elem_bytes, int64_t rows, int cols, int offset, const int32_t* cdf, int n,
                             int broadcast_rows, int precision, uint8_t* out, int64_t cap, int64_t* out_len);
/* coder_ops.range_decode (entropy_model.py:298; conditional_entropy_model.py:195). */
int pcgc_range_decode(const uint8_t* str, int64_t len, int64_t rows, int cols, const int32_t* cdf,
                      int n, int broadcast_rows, int precision, int16_t* out);
/* Same, publishing the number of completed rows in *progress (release stores, every 1024 rows and at the end; -1 on a
 * corrupt stream): the single z stream of a file is sequential (entropy_model.py:249-259), so its consumers start on
 * the first cubes' symbols while a helper thread is still decoding the rest. */
int pcgc_range_decode_progress(const uint8_t* str, int64_t len, int64_t rows, int cols, const int32_t* cdf,
                               int n, int broadcast_rows, int precision, int16_t* out, int64_t* progress);

/* Batched forms used by compress_hyper / decompress_hyper: n_streams independent
 * cubes coded on n_threads host threads (each stream stays sequential).
 * Encode consumes the device-produced lohi words (pcgc_laplace_cdf), sym_per_stream
 * per cube; out is n_streams slots of cap_per_stream bytes; out_lens[n_streams]. */
int pcgc_range_encode_lohi_batch(const uint32_t* lohi, int n_streams, int64_t sym_per_stream,
                                 int precision, uint8_t* out, int64_t cap_per_stream,
                                 int64_t* out_lens, int n_threads);
/* Decode consumes the device-produced uint16 lower-CDF rows [n_streams*sym_per_stream, ncols];
 * n_sym[s] = number of valid symbols (max-min+1) of stream s. Output int16 symbols. */
int pcgc_range_decode_u16_batch(const uint8_t* strings, const int64_t* offsets, const int64_t* lens,
                                int n_streams, int64_t sym_per_stream, const uint16_t* cdf_lower,
                                int ncols, const int32_t* n_sym, int precision, int16_t* out,
                                int n_threads);

/* load_points partition (dataprocess/inout_points.py:50-90) on an in-memory cloud.
 * points int32 [n,3].  Two-call protocol: first call with outputs NULL returns the
 * number of surviving cubes in *n_cubes; second call fills
 *   cube_positions int64 [n_cubes,3]  (first-appearance order, as the reference returns it)
 *   sorted_positions int64 [n_cubes,3] (key order = order of the cubes)
 *   cube_of_point int32 [n] (index into the SORTED cube list, -1 if its cube was dropped)
 *   points_numbers (unique voxels per cube, uint16 wrap like process.py:45). */
int pcgc_partition(const int32_t* points, int64_t n, int cube_size, int min_num, int64_t* n_cubes,
                   int64_t* cube_positions, int64_t* sorted_positions, int32_t* cube_of_point);

/* load_ply_data (dataprocess/inout_points.py:8-28) on a whole file image: every line whose first three
 * single-space-separated tokens read as Python floats is a point (header lines do not and are skipped, as are lines
 * with fewer than three tokens, where the reference raises), truncated to int32 like ndarray.astype.  out holds
 * cap x 3 values (cap >= number of lines is always enough); *n_points receives the count. */
int pcgc_parse_ply_points(const char* text, int64_t len, int32_t* out, int64_t cap, int64_t* n_points, int n_threads);

/* Body of write_ply_data (dataprocess/inout_points.py:43-44) for integer coordinates: "x y z\n" per point, digits
 * as Python's str(int).  *out_len always receives the exact text length (never more than 63 bytes per point); with a
 * smaller cap (or out == NULL) nothing is written and the call returns -2. */
int pcgc_format_points_int(const int64_t* pts, int64_t n, char* out, int64_t cap, int64_t* out_len);

/* Named numeric columns of an ASCII ply body (what follows the end_header line): every line that is not blank is a row of
 * whitespace-separated numbers, and out[row * k + j] receives the value of token columns[j] (0-based, in header order of
 * the properties) as a double.  At most max_rows rows are read (< 0: all; the vertex count of the header, so that face
 * lists are not taken for vertices).  out holds cap x k values; *n_rows always receives the count, and with a smaller
 * cap nothing is written and the call returns -2.  A row with too few tokens, or a token that is not a number, is an
 * error (-3) that names the line. */
int pcgc_parse_ply_columns(const char* text, int64_t len, const int32_t* columns, int k, int64_t max_rows, double* out,
                           int64_t cap, int64_t* n_rows, int n_threads);

/* Body of a coloured ply for integer coordinates: "x y z r g b\n" per point, digits as Python's str(int); pts int64
 * [n,3], colors uint8 [n,3].  Same protocol as pcgc_format_points_int. */
int pcgc_format_points_colors_int(const int64_t* pts, const uint8_t* colors, int64_t n, char* out, int64_t cap,
                                  int64_t* out_len);

/* o3d.io.read_triangle_mesh (mesh2pc_open3d.py:58) for the two formats the reference feeds it: format 0 = OFF
 * (ModelNet40, including its "OFF490 518 0" first line with the counts glued to the magic; extra per-vertex or per-face
 * values are ignored), 1 = OBJ (ShapeNet: `v x y z`, `f` with a, a/b, a//c, a/b/c corners and negative indices relative
 * to the vertices read so far; '#' starts a comment; other records are skipped).  Polygons are fan-triangulated
 * (0, i, i+1); faces with fewer than three corners add nothing; an index outside the vertices is an error (-3).
 * vertices double [vcap,3], triangles int32 [tcap,3]; *n_vertices / *n_triangles always receive the counts, and with
 * too small a capacity (or NULL outputs) nothing is written and the call returns -2. */
int pcgc_parse_mesh(const char* text, int64_t len, int format, double* vertices, int64_t vcap, int32_t* triangles,
                    int64_t tcap, int64_t* n_vertices, int64_t* n_triangles);
/* Triangle areas and their inclusive running sum in double, sequential like np.cumsum (sample_points_uniformly's
 * area weights): e = v1 - v0, f = v2 - v0, c = e x f (cx = ey fz - ez fy, ...), area = 0.5 sqrt((cx^2 + cy^2) + cz^2).
 * A total area of 0 is an error (-3). */
int pcgc_mesh_area_cdf(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double* cdf);

/* CRC-32C (Castagnoli, reflected 0x82F63B78), the checksum of TensorFlow's tensor-bundle checkpoints
 * (tf.train.Checkpoint files restored at transform.py:107-112; written at train_hyper.py:255-268).
 * Returns the crc of `crc_in`-continued data (pass 0 to start); not masked. */
uint32_t pcgc_crc32c(uint32_t crc_in, const void* data, int64_t n);

/* Reproducible elementary functions behind every pmf that becomes a range-coder CDF (Laplace:
 * conditional_entropy_model.py:21-56, 95-124; factorized: entropy_model.py:72-98, 114-151, 183-221).
 * They are fixed sequences of IEEE-754 binary32 +, -, *, /, floor (no FMA), written out in
 * pcgcv1_amd/csrc/repro_math.h and restated in numpy by oracle/entropy.py, so the HIP kernels, this host
 * library and the oracle produce identical bits; a stream written on one ROCm version decodes on another.
 *   fn: 0 exp, 1 log (normal x > 0), 2 tanh, 3 sigmoid, 4 softplus.   y[i] = fn(x[i]).
 * pcgc_host_repro_eval: libpcgc_host.so (CPU);  pcgc_repro_eval: libpcgc_hip.so (device pointers). */
int pcgc_host_repro_eval(int fn, const float* x, float* y, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* PCGC_H_ */
