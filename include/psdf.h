/* psdf.h -- C ABI of libpsdf_hip.so, the MI355X (gfx950) implementation of the PermutoSDF rendering/training hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  Each entry point replaces one
 * operator of the reference's Python-facing API -- the pybind11 module `permuto_sdf` (src/PyBridge.cxx:36-166) and
 * the external `permutohedral_encoding` package -- and cites the reference interface it stands in for.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 / int32 / 1-byte-bool data unless marked "host";
 *   - the callee never allocates and never synchronises: outputs are caller-allocated (zero-filled where a comment
 *     says "accumulated into" or where the reference allocates with torch::zeros), launches are asynchronous on `stream`
 *     (a hipStream_t; pass the framework's current stream, NULL = default stream);
 *   - return value: 0 = ok, -1 = argument error, -2 = unsupported configuration, > 0 = hipError_t of the launch;
 *   - ray-index arguments (nr_rays, ray_start_end_idx [R,2] int32, rays_have_equal_nr_of_samples,
 *     fixed_nr_of_samples_per_ray, max_nr_samples) mirror RaySamplesPacked (include/permuto_sdf/RaySamplesPacked.cuh:6-46);
 *   - PCG32 generators are passed by value as (state, inc) exactly as the reference passes `pcg32 rng` to its kernels;
 *     the owner advances its host copy by 2^32 after every jittered call (src/OccupancyGrid.cu:252-254).
 */
#ifndef PSDF_H
#define PSDF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- encode.hip ---- */
/* The frozen conventions of the encoding (upstream source absent, PARITY UNPINNED) are the #defines of
   permuto_sdf_amd/csrc/encode_conventions.h; `concat_points` below is one of PSDF_ENC_CONCAT_NONE (0),
   PSDF_ENC_CONCAT_PSEUDO_LEVELS (1: F*(L + ceil(P/F)) channels, zero padded) or PSDF_ENC_CONCAT_APPEND (2: F*L + P channels,
   `cat([sliced, scaling * points])`, what permuto_sdf_py/models/models.py:149,154 consumes through output_dims()).
   psdf_encode_convention(i) returns the value IN FORCE of convention i (0 hash multiplier, 1 rank tie rule -- the two that
   live in device code, runtime values -- 2 sqrt term of scale_factor, 3 inverse-std-dev term, 4 default concatenation layout --
   host-side defaults: `scale_factor` and `concat_points` are arguments of every entry point); host only.
   psdf_encode_set_conventions() replaces the two device-side ones for the process (kernel arguments from then on), so that
   matching an upstream build that disagrees with the recollection is a flag flip, not a rebuild (INTEGRATION.md,
   tools/dump_upstream_encoding_vectors.py, tests/test_upstream_vectors.py).  No reference counterpart. */
int64_t psdf_encode_convention(int which);
int psdf_encode_set_conventions(uint32_t hash_multiplier, int rank_tie_raises_later);

/* The launch form of the encode forward for this process: a grid row per level (0), or coarse levels handled together with
   fine ones, `pairs` of them (n > 0, clamped to nr_levels / 2 per call; -1: the library's default rule, also what
   PSDF_ENC_FWD_PAIRS sets at start-up).  A speed setting only: the outputs are bit-identical in every form.  -1 (argument
   error) below -1.  No reference counterpart. */
int psdf_encode_set_forward_pairs(int pairs);

/* replaces: permutohedral_encoding CUDA op `forward_gpu` (un-vendored; call sites permuto_sdf_py/models/models.py:186,370,500,542)
   -2 (unsupported) when one level of the table exceeds 4 GiB (capacity * nr_feat * 4 bytes: the kernel gathers with 32-bit
   offsets from the level's base; the reference's tables are 2 MiB per level) */
int psdf_encode_forward(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
    const float* lattice, const float* scale_factor, const float* shifts, const float* window, int concat_points,
    float points_scaling, float* sliced, void* stream);

/* same operator; additionally sets touched_blocks[level][row >> block_rows_log2] = 1 for every table row the batch reads
   (bytes, [nr_levels, ceil(capacity / 2^block_rows_log2)], never cleared here): what psdf_adamw_step_blocks consumes */
int psdf_encode_forward_mark(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
    const float* lattice, const float* scale_factor, const float* shifts, const float* window, int concat_points,
    float points_scaling, float* sliced, unsigned char* touched_blocks, int block_rows_log2, void* stream);

/* replaces: permutohedral_encoding `backward_gpu` / `backward_gpu_only_pos` (autograd of models.py:186; positions grad needed by models.py:240-251) */
int psdf_encode_backward(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
    const float* lattice, const float* scale_factor, const float* shifts, const float* window, int concat_points,
    float points_scaling, const float* grad_sliced, float* grad_lattice, float* grad_positions, void* stream);

/* same operator with caller-provided device scratch: enables the binned queue + LDS-reduction lattice-gradient path
   for large batches (psdf_encode_backward_workspace_bytes() == 0 means "not applicable", pass NULL) */
int64_t psdf_encode_backward_workspace_bytes(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity);
int psdf_encode_backward_ws(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
    const float* lattice, const float* scale_factor, const float* shifts, const float* window, int concat_points,
    float points_scaling, const float* grad_sliced, float* grad_lattice, float* grad_positions, void* workspace,
    int64_t workspace_bytes, void* stream);
/* debug query: how the last balanced binning launch of psdf_encode_backward_ws dealt its resident round of workgroups over the
   levels (counts[0 .. nr_levels)); returns nr_levels, 0 when no balanced launch has run.  Shares follow the measured duration
   of each level's workgroups in the previous call (PSDF_ENC_BWD_BALANCE=0: equal shares); closed levels fall to the minimum.
   REPRODUCIBILITY: the deal -- and with it the order of the float additions of the lattice gradient -- depends on the timing of
   the previous call; PSDF_ENC_BWD_BALANCE=0 is the switch for run-to-run comparisons (state is kept per device, lattice and
   shape class).  NON-FINITE INPUTS: contributions of neighbouring samples to one table row are merged in registers with
   multiply-adds (encode.hip, combine_runs16), so ONE non-finite upstream gradient makes the gradient of up to 15 other table
   rows handled by the same 16 lanes NaN as well -- a NaN batch is a NaN batch, but more rows show it than carry it. */
int psdf_encode_backward_level_shares(int* counts, int max_levels);
/* debug query: how the binning workgroups of the last queue-path call (backward or double backward) that used `workspace` left
   their LDS scatter caches, per level: kept[l] kept the cache to the end of their walk and handed it to the queues in one
   round, voted_off[l] switched it off after their first super-tile.  The shape arguments are those of that call.  Waits for
   `stream`.  Returns the levels written (at most 64 and max_levels); 0 when the queue plan does not apply. */
int psdf_encode_backward_cache_votes(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const void* workspace,
    int64_t workspace_bytes, int* kept, int* voted_off, int max_levels, void* stream);


/* replaces: permutohedral_encoding `double_backward_from_positions_gpu` (create_graph=True at models.py:245-251) */
int psdf_encode_double_backward(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float*
    positions, const float* lattice, const float* scale_factor, const float* shifts, const float* window, int
    concat_points, float points_scaling, const float* dd_positions, const float* grad_sliced, float* grad_lattice,
    float* grad_grad_sliced, void* stream);
/* Same, with the backward's device workspace (psdf_encode_backward_workspace_bytes; NULL = none): large batches send the
 * lattice scatter through the binning + reduce kernels instead of float atomics.  grad_grad_sliced may be NULL when only the
 * lattice gradient is wanted.  grad_sliced_direct (optional, [C, N]): the lattice scatter of the PLAIN backward for this upstream
 * gradient is added in the same pass (grad_lattice += d<sliced, grad_sliced_direct>/d lattice): a training step sends both onto
 * the same rows. */
int psdf_encode_double_backward_ws(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
                                   const float* lattice, const float* scale_factor, const float* shifts, const float* window,
                                   int concat_points, float points_scaling, const float* dd_positions, const float* grad_sliced,
                                   float* grad_lattice, float* grad_grad_sliced, const float* grad_sliced_direct,
                                   void* workspace, int64_t workspace_bytes, void* stream);

/* ---- mlp.hip, opt-in arithmetic ---- */
/* psdf_mlp_pack / psdf_mlp_forward with TWO fp16 pieces per fp32 operand (three products on v_mfma_f32_32x32x16_f16) instead of
   three bf16 pieces (six products): the BASELINE net only (dims = {<= 64, 64, 64, 64, <= 4}: baseline_split_shape of csrc/mlp_dispatch.h; -2 otherwise); max error ~3e-6 of
   the largest output instead of ~1e-6; inputs, activations and weights must stay below 65504 in magnitude.  A buffer made by
   psdf_mlp_pack_f16 is consumed by psdf_mlp_forward_f16 only. */
int psdf_mlp_pack_f16(int n_layers, const int* dims, const float* const* weights, const float* const* biases, float* packed,
    void* stream);
int psdf_mlp_forward_f16(int n_layers, const int* dims, int64_t N, const float* X, const float* packed, float* Y, void* stream);

/* Test and A/B hook of the split forward kernels (psdf_mlp_forward, _masked and _f16 where they take the split-operand kernel):
   psdf_mlp_forward_set_form forces the workgroup form, `waves` per workgroup sharing one weight image (4, 8 or 16; 0 = the
   launch policy picks by batch size again; -1 for any other value), for the process until it is called again.  A forward whose
   net has no kernel of the forced form returns -2 and launches nothing.  psdf_mlp_forward_last_form: the waves per workgroup of
   the last split forward launch (0: none yet); psdf_last_path(2) keeps naming the arithmetic.  No reference counterpart. */
int psdf_mlp_forward_set_form(int waves);
int psdf_mlp_forward_last_form(void);

/* ---- composite_fused.hip ---- */
/* replaces, fused: VolumeRenderingNeus.compute_weights + integrate (permuto_sdf_py/volume_rendering/volume_rendering_modules.py:
   129-190), i.e. the chain psdf_neus_alpha_forward -> psdf_cumprod_alpha2transmittance -> (alpha * T) ->
   psdf_integrate_with_weights in ONE launch: pred [R,3] (every ray written: 0 for invalid / empty rays), bg [R] (optional; 1 for
   such rays), weights [N] (optional).  Same arithmetic and summation order as the separate entry points. */
int psdf_neus_composite_forward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* sdf,
    const float* dirs, const float* gradients, const float* dt, const float* rgb, const float* inv_s, float cos_anneal_ratio,
    float* pred, float* bg, float* weights, void* stream);
/* its backward in one launch (integrate_with_weights_backward, the transmittance backward with its inverse cumulative sum,
   the opacity backward: volume_rendering_funcs.py:55-190): grad_pred [R,3], grad_bg [R] or NULL -> grad_sdf [N]; optional
   grad_gradients [N,3], grad_rgb [N,3], grad_inv_s [1] (accumulated into).  max_per_ray = an upper bound of the samples of any
   ray, at most 256 (-2 beyond: use the per-operator entry points); reference_compat as in psdf_integrate_with_weights_backward. */
int psdf_neus_composite_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int max_per_ray,
    const float* grad_pred, const float* grad_bg, const float* sdf, const float* dirs, const float* gradients, const float* dt,
    const float* rgb, const float* inv_s, float cos_anneal_ratio, int reference_compat, float* grad_sdf, float* grad_gradients,
    float* grad_rgb, float* grad_inv_s, void* stream);

/* Background NeRF (NerfHash + VolumeRenderingNerf.compute_weights + integrate: models.py:520, volume_rendering_modules.py:72-86,
   176-190) and the composition with the foreground (train_permuto_sdf.py:160-165), one launch per direction:
   density = softplus(raw_density); alpha = 1 - exp(-density dt); T = exclusive cumprod(1 - alpha + 1e-7); w = alpha T;
   pred_bg [R,3] = sum w rgb; with fg_pred [R,3] and fg_bg [R] (both or neither) also pred [R,3] = fg_pred + fg_bg * pred_bg. */
int psdf_nerf_composite_forward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* raw_density,
                                const float* dt, const float* rgb, const float* fg_pred, const float* fg_bg, float* pred_bg,
                                float* pred, void* stream);
/* its backward for grad_pred [R,3] (of the composed radiance when fg_bg is given, else of pred_bg): grad_raw_density [M], grad_rgb
   [M,3], optional grad_fg_bg [R] = <grad_pred, pred_bg>; rays of at most max_per_ray <= 256 samples (-2 beyond) */
int psdf_nerf_composite_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int max_per_ray,
                                 const float* grad_pred, const float* fg_bg, const float* raw_density, const float* dt,
                                 const float* rgb, int reference_compat, float* grad_raw_density, float* grad_rgb,
                                 float* grad_fg_bg, void* stream);

/* ---- neus_render.hip ---- */
/* The NeuS render of a `--with_mask` training step (train_permuto_sdf.py:153-154,381-383): psdf_neus_composite_forward with the
   per-ray weight sum as a third output, its backward with a gradient into it, and the step's colour + mask loss in one call. */
/* host only: the launch plan (csrc/neus_render_plan.h) -> out [PSDF_NEUS_RENDER_PLAN_FIELDS] int64: 0 the register chunks K of
   the ray backward for max_per_ray (1, 2, 4); 1 workgroups of the loss kernel for nr_rays; 2 bytes of the workspace
   psdf_neus_mask_loss needs for nr_rays (0 up to the single-group limit); 3 that limit (8192 rays).
   -1: nr_rays < 0, max_per_ray < 1; -2: nr_rays > (2^31 - 1) / 3, max_per_ray > 256 */
#define PSDF_NEUS_RENDER_PLAN_FIELDS 4
int psdf_neus_render_plan(int64_t nr_rays, int max_per_ray, int64_t* out);
/* one launch, any ray length: pred [R,3], weights_sum [R] = sum alpha T, bg_transmittance [R]; each may be NULL (one at least is
   given; rgb may be NULL without pred).  Empty and overflowed rays: 0, 0, 1.  pred and bg_transmittance have the bits of
   psdf_neus_composite_forward. */
int psdf_neus_render_forward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* sdf,
    const float* dirs, const float* gradients, const float* dt, const float* rgb, const float* inv_s, float cos_anneal_ratio,
    float* pred, float* weights_sum, float* bg_transmittance, void* stream);
/* its backward in one launch for grad_pred [R,3], grad_weights_sum [R], grad_bg_transmittance [R] (each may be NULL, one at
   least is given) -> grad_sdf [N]; optional grad_gradients [N,3], grad_rgb [N,3], grad_inv_s [1] (accumulated into).
   max_per_ray, reference_compat, skipped rays: as psdf_neus_composite_backward, whose bits every output has when
   grad_weights_sum is NULL.  A ray longer than max_per_ray rounded up to 64 K comes back as NaN. */
int psdf_neus_render_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int max_per_ray,
    const float* grad_pred, const float* grad_weights_sum, const float* grad_bg_transmittance, const float* sdf, const float* dirs,
    const float* gradients, const float* dt, const float* rgb, const float* inv_s, float cos_anneal_ratio, int reference_compat,
    float* grad_sdf, float* grad_gradients, float* grad_rgb, float* grad_inv_s, void* stream);
/* loss[0] += scale_rgb * sum |pred - gt| hit[ray] + scale_mask * sum BCE(clip(weights_sum, 1e-3, 1 - 1e-3), gt_mask) over
   nr_rays rays (pred, gt [R,3]; hit [R] bytes or NULL; weights_sum, gt_mask [R]), and the gradients of that sum: grad_pred [R,3]
   as psdf_l1_loss writes it, grad_weights_sum [R] through the clip (passed on the closed interval, 0 outside); both optional.
   Deterministic, no floating-point atomics.  workspace: psdf_neus_render_plan's bytes (may be NULL when they are 0). */
int psdf_neus_mask_loss(int64_t nr_rays, const float* pred, const float* gt, const unsigned char* hit, const float* weights_sum,
    const float* gt_mask, float scale_rgb, float scale_mask, double* workspace, float* loss, float* grad_pred,
    float* grad_weights_sum, void* stream);

/* ---- debug query (mlp_bwd.hip) ---- */
/* Which kernel variant the LAST call of an operator family dispatched to (host only, no device work): lets a parity test
   assert that the configuration it compares with the oracle ran the kernels the benchmark times.  No reference counterpart.
     family 0 encode backward: 1 LDS scatter cache + atomics, 2 queue mode (binning + encode_bwd_reduce_kernel), 3 positions only
     family 1 MLP backward   : 1 fp32-MFMA kernel, 2 split-bf16 kernel (mlp_bwd_split.hip), 3 wide workgroup kernel,
                               4 split-fp16 kernel (mlp_bwd_split_f16.hip)
     family 2 MLP forward    : 1 fp32-MFMA kernel, 2 split-bf16 kernel, 3 split-fp16 kernel (psdf_mlp_forward_f16)
   0 = no call yet, -1 = unknown family. */
int psdf_last_path(int family);
/* Which MLP widths have a fused kernel (host only: no device work, no environment read).  op: one of PSDF_MLP_OP_*, naming an
   entry point: FORWARD psdf_mlp_forward(_masked), FORWARD_F16 psdf_mlp_forward_f16, FORWARD_WIDE_F16 psdf_mlp_forward_wide_f16,
   BACKWARD psdf_mlp_backward with dW / db, BACKWARD_DATA the same with dW = db = NULL, BACKWARD_DATA_MASKED
   psdf_mlp_backward_data_masked, DOUBLE_BACKWARD psdf_mlp_double_backward, DOUBLE_BACKWARD_PLUS psdf_mlp_double_backward_plus.
   1: a kernel is instantiated for these widths and the entry point launches it; 0: the entry point returns -2 for them; -1:
   argument error (unknown op, dims NULL, n_layers outside 2..5, a width <= 0).  Computed from the dispatch table the entry
   points expand (csrc/mlp_dispatch.h), LDS limits included.  It reports which kernels exist for the widths, not the runtime
   demotions: stream capture, PSDF_MLP_BWD_SPLIT / PSDF_MLP_WIDE_SPLIT, the fp16 range guard and the large-batch (N >= 2^18)
   split backward are not looked at -- so {K0 <= 16, 64, 64, 64, 1}, which only that split backward serves, answers 0. */
enum {
  PSDF_MLP_OP_FORWARD = 0,
  PSDF_MLP_OP_FORWARD_F16 = 1,
  PSDF_MLP_OP_FORWARD_WIDE_F16 = 2,
  PSDF_MLP_OP_BACKWARD = 3,
  PSDF_MLP_OP_BACKWARD_DATA = 4,
  PSDF_MLP_OP_BACKWARD_DATA_MASKED = 5,
  PSDF_MLP_OP_DOUBLE_BACKWARD = 6,
  PSDF_MLP_OP_DOUBLE_BACKWARD_PLUS = 7
};
int psdf_mlp_supported(int op, int n_layers, const int* dims);

/* ---- mlp_bwd_split.hip ---- */
/* same contract as psdf_mlp_backward for dims = {K0 <= 52, 64, 64, 64, 1} (baseline_split_shape of csrc/mlp_dispatch.h and
   the kernel's LDS limit) with dW/db requested, computed on the bf16 matrix
   pipe with split fp32 operands (three bf16 pieces, six products kept: fp32-level accuracy); -2 for every other net and when
   stream-ordered scratch is unavailable (stream capture).  psdf_mlp_backward routes large batches here by itself. */
int psdf_mlp_backward_split(int n_layers, const int* dims, int64_t N, const float* X, const float* const* weights,
    const float* const* biases, const float* dY, float* dX, float* const* dW, float* const* db, void* stream);

/* ---- mlp_bwd_split_f16.hip ---- */
/* same contract as psdf_mlp_backward for dims = {K0 <= 64, 64, 64, 64, 1} (baseline_split_shape of csrc/mlp_dispatch.h) with
   dW/db requested, computed on the fp16 matrix pipe
   with TWO fp16 pieces per fp32 operand (three products in the chains, four in the dW products); the gradient chain of every
   sample runs on the mantissa of its dY and the factor 2^e is restored exactly, so the accuracy does not depend on the size or
   spread of dY (errors of a few 1e-6 of the largest entry against float64; activations / weights must stay below 65504 in
   magnitude).  -2 for every other net and when stream-ordered scratch is unavailable.  psdf_mlp_backward routes large batches
   here by default (PSDF_MLP_BWD_SPLIT=bf16 selects psdf_mlp_backward_split instead). */
int psdf_mlp_backward_split_f16(int n_layers, const int* dims, int64_t N, const float* X, const float* const* weights,
    const float* const* biases, const float* dY, float* dX, float* const* dW, float* const* db, void* stream);
/* 1 once psdf_mlp_backward_split_f16 has launched mlp_bwd_split_f16_kernel (one wave per SIMD: the only form built since round 6;
   the two two-waves-per-SIMD forms of round 5 were slower and live in attic/rejected/), 0 = none yet.  Debug query (host only). */
int psdf_mlp_backward_split_f16_form(void);
/* range guard of the split-fp16 backward: inputs / hidden activations of magnitude >= 255 or weights >= 65504 leave the range
   of its two-piece arithmetic; such a batch is redone on the device by the three-piece bf16 kernel (K0 <= 52; no host
   round trip) and counted here -- the number of launches that raised the guard so far (exact after a synchronisation).
   The first such event also prints one line to stderr at the next call. */
unsigned psdf_mlp_f16_range_events(void);

/* ---- mlp_wide.hip ---- */
/* (also, round 6: the background density / feature net 52 -> 64 x 3 -> 65, models.py:451-459: dims[0] <= 64, 32 < dims[1..3] <= 64,
   16 < dims[4] <= 80 -- density_net_shape of csrc/mlp_dispatch.h)
   Forward of the reference's colour network shape (LipshitzMLP 111 -> 128 -> 128 -> 64 -> 3, models.py:54-129,349-350: dims[0] <= 112,
   dims[1], dims[2] <= 128, dims[3] <= 64, dims[4] <= 16: colour_net_shape of csrc/mlp_dispatch.h) on the fp16 matrix pipe with two pieces per fp32 operand: X [dims[0], N],
   Y [dims[4], N] feature-major; weights[l] [dims[l+1], dims[l]] (for a LipshitzMLP the NORMALISED weights), biases[l]; GELU between
   the layers, the last one linear.  N == 0: PSDF_OK before any pointer is looked at, nothing touched.  -2: another shape, stream
   capture, PSDF_MLP_WIDE_SPLIT=f32, or a value beyond the fp16 range met by an earlier launch (psdf_mlp_forward evaluates every shape
   with fp32 MFMAs).  Range guard: an input, hidden activation or weight of magnitude >= 32768 raises this launch's guard word; the
   same launch then redoes the batch with fp32 MFMAs on the device (Y is exact to the fp32 kernel's bar, never inf / NaN from the
   split), and raises the process-wide switch that makes later calls return -2. */
int psdf_mlp_forward_wide_f16(int n_layers, const int* dims, int64_t N, const float* X, const float* const* weights,
    const float* const* biases, float* Y, void* stream);
/* which kernel the last psdf_mlp_backward_wide launched: 1 = fp32 MFMAs (mlp_wide_bwd_kernel), 2 = two fp16 pieces per operand on
   the fp16 matrix pipe (mlp_wide_bwd_f16_kernel, the default since round 6; PSDF_MLP_WIDE_SPLIT=f32 selects the other, and so does a
   value beyond the fp16 range met by an earlier launch); 0 = none yet.  Debug query (host only). */
int psdf_mlp_backward_wide_form(void);
/* same contract as psdf_mlp_backward for 4-layer nets wider than one wave's register file holds (dims[0] <= 112, dims[1],
   dims[2] <= 128, dims[3] <= 64, dims[4] <= 16: colour_net_shape of csrc/mlp_dispatch.h): the colour network LipshitzMLP 111 -> 128 -> 128 -> 64 -> 3 of
   permuto_sdf_py/models/models.py:54-129,349-350 (weights = the already normalised ones).  Workgroup-cooperative: 8 waves
   share a 32-sample tile through LDS, each owns one output tile per layer.  -2 for other widths / no stream-ordered scratch;
   psdf_mlp_backward falls through to it.  Also (split-fp16 kernel only): the 64-wide nets with many outputs (background density
   net 52 -> 64 x 3 -> 65, models.py:451-459: density_net_shape, hidden layers of 33..64) and, with n_layers = 3, the background colour head 80 -> 64 -> 64 -> 3
   (models.py:463-469: 64 < dims[0] <= 80, 48 < dims[1], dims[2] <= 64, dims[3] <= 4: the heads the single-wave fp32 redo covers; colour_head_shape).  N == 0: PSDF_OK before any pointer is
   looked at, nothing touched.  Range guard of the split-fp16 kernel: |input| >= 32, |hidden activation| >= 128 (the H side of the
   parameter-gradient products is pre-scaled by 2^10 / 2^8), |dZ of the per-sample scaled chain| >= 32768 or |weight| >= 32768
   raise the launch's own guard word: its gradient images are dropped and the fp32 kernel (4 layers: mlp_wide_bwd_kernel; 3: the
   single-wave head kernel) queued behind it -- a no-op otherwise -- redoes the batch in the same call; the process-wide switch goes
   up with it, and later calls take the fp32 kernel outright (psdf_mlp_backward_wide_form() == 1). */
int psdf_mlp_backward_wide(int n_layers, const int* dims, int64_t N, const float* X, const float* const* weights,
    const float* const* biases, const float* dY, float* dX, float* const* dW, float* const* db, void* stream);

/* replaces: LipshitzMLP.normalization (models.py:98-104): Wn[r][:] = W[r][:] * min(1, softplus(c[0]) / sum_j |W[r][j]|), and its
   autograd (grad_W written, grad_c[0] accumulated into) */
int psdf_lipshitz_normalize_forward(int out, int in, const float* W, const float* c, float* Wn, void* stream);
int psdf_lipshitz_normalize_backward(int out, int in, const float* W, const float* c, const float* grad_Wn, float* grad_W,
    float* grad_c, void* stream);
/* all layers of a LipshitzMLP (n_layers <= 8) in one launch per direction: W[l] [out[l], in[l]], c[l] [1] on the device */
int psdf_lipshitz_normalize_forward_multi(int n_layers, const int* out, const int* in, const float* const* W, const float* const* c,
                                          float* const* Wn, void* stream);
int psdf_lipshitz_normalize_backward_multi(int n_layers, const int* out, const int* in, const float* const* W, const float* const* c,
                                           const float* const* grad_Wn, float* const* grad_W, float* const* grad_c, void* stream);

/* ---- neus.hip ---- */
/* replaces: the torch elementwise chain of VolumeRenderingNeus.compute_weights, permuto_sdf_py/volume_rendering/
   volume_rendering_modules.py:129-172 (cos anneal, section-point SDFs, two sigmoids, (p+1e-5)/(c+1e-5) clipped to [0,1]);
   inv_s is a DEVICE pointer to one float (the clipped exp(10*variance) of SingleVarianceNetwork, :96-115), samples are the
   packed [N,1]/[N,3] tensors of RaySamplesPacked; one_minus_alpha (optional) = 1 - alpha + 1e-7, the transmittance input */
int psdf_neus_alpha_forward(int64_t N, const float* sdf, const float* dirs, const float* gradients, const float* dt,
    const float* inv_s, float cos_anneal_ratio, float* alpha, float* one_minus_alpha, void* stream);
/* replaces: torch autograd of the same chain.  grad_gradients [N,3] and grad_inv_s [1] are optional; grad_inv_s is
   ACCUMULATED into (zero it first) */
int psdf_neus_alpha_backward(int64_t N, const float* grad_alpha, const float* sdf, const float* dirs, const float*
    gradients, const float* dt, const float* inv_s, float cos_anneal_ratio, float* grad_sdf, float* grad_gradients,
    float* grad_inv_s, void* stream);
/* replaces: rgb_loss, permuto_sdf_py/utils/permuto_sdf_utils.py:43-47: loss[0] += scale * sum |gt - pred| * mask[ray]
   (mask: optional [R] bytes), grad_pred (optional) = scale * sign(pred - gt) * mask */
int psdf_l1_loss(int64_t R, int C, const float* pred, const float* gt, const unsigned char* mask, float scale,
    float* loss, float* grad_pred, void* stream);
/* replaces: eikonal_loss, permuto_sdf_utils.py:49-51: loss[0] += scale * sum (|g| - 1)^2, grad (optional) [N,3] */
int psdf_eikonal_loss(int64_t N, const float* gradients, float scale, float* loss, float* grad_gradients, void* stream);
/* replaces: F.normalize(x, dim=-1) and its autograd backward (torch), used on the SDF gradients at
   permuto_sdf_py/models/models.py:272,280,367: grad_y == NULL -> out = x / max(|x|, 1e-12); else out = d/dx applied to grad_y */
int psdf_normalize3(int64_t N, const float* x, const float* grad_y, float* out, void* stream);
/* sigmoid at the end of the colour heads (models.py:386,525), fused with the layout change the compositing operators need:
   y [N, C] = sigmoid(x_fm [C, N]);  grad_x_fm [C, N] = grad_y [N, C] * y * (1 - y);  C <= 16 */
int psdf_sigmoid_rows(int64_t N, int C, const float* x_fm, float* y, void* stream);
int psdf_sigmoid_rows_backward(int64_t N, int C, const float* grad_y, const float* y, float* grad_x_fm, void* stream);
/* replaces: the shifted points of the curvature loss, models.py:266-277: out = points + epsilon * cross(normalize(gradients),
   normalize(rand_directions)) (grad_shifted == NULL), or the gradient of that w.r.t. `gradients` applied to grad_shifted */
int psdf_curvature_shift(int64_t N, const float* points, const float* gradients, const float* rand_directions, float
    epsilon, const float* grad_shifted, float* out, void* stream);
/* replaces: models.py:280-289 + the mean at train_permuto_sdf.py:363: loss[0] += scale * sum acos(clamp(n(g) . n(g_shifted),
   -1+1e-6, 1-1e-6)) / pi; the two gradient outputs are optional (both or none) */
int psdf_curvature_loss(int64_t N, const float* gradients, const float* gradients_shifted, float scale, float* loss,
    float* grad_gradients, float* grad_gradients_shifted, void* stream);
/* replaces: the off-surface loss, train_permuto_sdf.py:372-375: loss[0] += scale * sum exp(-sharpness |sdf|) */
int psdf_offsurface_loss(int64_t N, const float* sdf, float sharpness, float scale, float* loss, float* grad_sdf, void*
    stream);
/* replaces: NerfHash density activation + VolumeRenderingNerf alpha, models.py:520 (softplus) and
   volume_rendering_modules.py:72-86: alpha = 1 - exp(-softplus(raw) dt), one_minus_alpha = 1 - alpha + 1e-7 */
int psdf_nerf_alpha_forward(int64_t N, const float* raw_density, const float* dt, float* alpha, float* one_minus_alpha,
    void* stream);
int psdf_nerf_alpha_backward(int64_t N, const float* raw_density, const float* dt, const float* grad_alpha, const float*
    grad_one_minus_alpha, float* grad_raw_density, void* stream);

/* ---- mlp.hip ---- */
/* replaces: torch.nn.Sequential(Linear,GELU,...) evaluators, permuto_sdf_py/models/models.py:153-161,451-470 */
int64_t psdf_mlp_packed_size(int n_layers, const int* dims);

/* replaces: same evaluators (parameter re-ordering for the MFMA kernels).  `packed` holds psdf_mlp_packed_size floats:
   the fp32 operand image and, for nets whose image fits 80 KB of LDS, a second image of the same parameters as three
   bf16 pieces per weight (16-byte aligned, after the first) that psdf_mlp_forward multiplies on the bf16 matrix pipe
   with six products kept per fp32 multiply (fp32-level accuracy; no range restriction on inputs or weights). */
int psdf_mlp_pack(int n_layers, const int* dims, const float* const* weights, const float* const* biases, float*
    packed, void* stream);

/* replaces: models.py:187 `self.mlp_sdf(point_features)` and :508-517 (cuBLAS + elementwise GELU in the reference) */
int psdf_mlp_forward(int n_layers, const int* dims, int64_t N, const float* X, const float* packed, float* Y, void*
    stream);

/* ---- encode.hip / mlp.hip: masked forward ---- */
/* per-sample masks for fixed-shape callers (one slot per ray: the sphere tracer's converged rays): masked points /
   fully masked 32-sample tiles are not evaluated, their outputs are left untouched */
int psdf_encode_forward_masked(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
    const float* lattice, const float* scale_factor, const float* shifts, const float* window, int concat_points, float
    points_scaling, const uint8_t* skip, float* sliced, void* stream);
int psdf_mlp_forward_masked(int n_layers, const int* dims, int64_t N, const float* X, const float* packed, const uint8_t*
    skip, float* Y, void* stream);
/* the analytic normal of the same callers (reference: get_sdf_and_gradient on the traced end points,
   permuto_sdf_py/utils/sdf_utils.py:203-208, which in the reference holds only the rays that met occupancy): data gradient
   of the MLP and position gradient of the encoding under the same mask; masked samples keep the contents of their outputs */
int psdf_mlp_backward_data_masked(int n_layers, const int* dims, int64_t N, const float* X, const float* const* weights,
    const float* const* biases, const float* dY, const uint8_t* skip, float* dX, void* stream);
int psdf_encode_backward_positions_masked(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float*
    positions, const float* lattice, const float* scale_factor, const float* shifts, const float* window, int
    concat_points, float points_scaling, const float* grad_sliced, const uint8_t* skip, float* grad_positions, void*
    stream);
/* the same with the caller's scratch for the per-level-group partial sums: they are added in group order, never with float
   atomics, so the same inputs give the same bits on every call, also while `stream` is being captured into a graph (where the
   entry above has no scratch of its own and takes the atomic form).  Outside a capture the bits are the entry's above.
   replaces: nothing new in the reference (the same get_sdf_and_gradient); what it adds is a captured trace whose normals equal
   the eager trace's bit for bit (box_trace.py).  workspace: psdf_encode_backward_positions_workspace_bytes() bytes (host only;
   0: none needed, workspace may be NULL); a smaller or missing workspace: -1 */
int64_t psdf_encode_backward_positions_workspace_bytes(int pos_dim, int nr_feat, int64_t N, int nr_levels, int concat_points);
int psdf_encode_backward_positions_masked_ws(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float*
    positions, const float* lattice, const float* scale_factor, const float* shifts, const float* window, int
    concat_points, float points_scaling, const float* grad_sliced, const uint8_t* skip, float* grad_positions, void*
    workspace, int64_t workspace_bytes, void* stream);

/* ---- mlp_bwd.hip ---- */
/* replaces: autograd backward of the same evaluators (dX, dW_l, db_l in one launch; forward recomputed from X).
   weights[l]/biases[l]: torch-layout parameters; dW[l]/db[l] are accumulated into (caller zero-fills); dW = db = NULL:
   data gradient only (lighter kernel: analytic normals at inference).  dY = NULL (data gradient only; also accepted by
   psdf_mlp_backward_data_masked and psdf_mlp_double_backward): the unit gradient of output 0, i.e. d y_0 / d X -- the
   `torch.autograd.grad(sdf, points, torch.ones_like(sdf))` of models.py:236-251 without a [rows, N] tensor that is 1 in one row */
int psdf_mlp_backward(int n_layers, const int* dims, int64_t N, const float* X, const float* const* weights, const
    float* const* biases, const float* dY, float* dX, float* const* dW, float* const* db, void* stream);

/* replaces: the second differentiation torch autograd performs for the reference's eikonal / curvature losses
   (get_sdf_and_gradient with create_graph=True, models.py:236-251): VJP of (X, params) -> dX = J^T dY with upstream
   gradient V [dims[0], N]; dX2 receives d/dX, dW[l] / db[l] are accumulated into; 3 hidden layers */
int psdf_mlp_double_backward(int n_layers, const int* dims, int64_t N, const float* X, const float* const* weights,
    const float* const* biases, const float* dY, const float* V, float* dX2, float* const* dW, float* const* db,
    void* stream);
/* the same pass with the plain backward of an upstream gradient dY2 [dims[n_layers], N] of the net's OUTPUTS folded in (round 6: the
   training step runs both on the same samples -- g_y of (sdf, geometry features) beside g_n of the normals; one forward
   recomputation, one backward sweep, one launch instead of psdf_mlp_backward + psdf_mlp_double_backward): dX2 = the double
   backward's data gradient + the dX psdf_mlp_backward would return for dY2; dW[l] / db[l] accumulate both.  The reference's SDF net
   shapes only (models.py:153-161: <= 64 inputs, 32 x 3 hidden, a matrix output layer of 5 .. 48 rows); -2 otherwise */
int psdf_mlp_double_backward_plus(int n_layers, const int* dims, int64_t N, const float* X, const float* const* weights,
    const float* const* biases, const float* dY, const float* V, const float* dY2, float* dX2, float* const* dW,
    float* const* db, void* stream);

/* ---- fused.hip ---- */
/* replaces: models.py:186-192 `point_features=self.encoding(points, window); sdf_and_feat=self.mlp_sdf(point_features)`
   as ONE launch that never materialises the feature tensor (pos_dim 3, 2 features/level).  dims[0] must be
   2*(nr_levels + (concat_points?2:0)); skip [N] bytes and feat [dims[0],N] are optional (NULL) */
int psdf_encode_mlp_forward(int64_t N, int nr_levels, int capacity, const float* positions, const float* lattice,
    const float* scale_factor, const float* shifts, const float* window, int concat_points, float points_scaling,
    int n_layers, const int* dims, const float* packed, const uint8_t* skip, float* feat, float* Y, void* stream);

/* ---- optim.hip ---- */
/* replaces: torch.optim.AdamW at permuto_sdf_py/train_permuto_sdf.py:293-304,418 */
int psdf_adamw_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float
    beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* the same update for up to 64 tensors sharing the step count, one launch (host arrays of sizes / device pointers) */
int psdf_adamw_step_multi(int n_tensors, const int64_t* sizes, float* const* params, const float* const* grads, float*
    const* exp_avgs, float* const* exp_avg_sqs, float lr, float beta1, float beta2, float eps, float weight_decay, int
    step, float grad_scale, void* stream);

/* replaces: the same dense update (train_permuto_sdf.py:293-304: weight_decay 0 on the lattices) restricted to the blocks
   where it is not the identity.  The tensor is n_blocks blocks of block_elems floats; a block whose gradient and both
   moments are exactly zero (no batch ever touched its rows) is skipped, every other block gets the dense update -- moments
   of rows a batch does NOT touch keep decaying, as in torch.  touched [n_blocks] bytes: from psdf_encode_forward_mark,
   consumed (reset to 0); active [n_blocks] bytes: 1 once a block has been updated; zero_grad != 0: the gradient of the
   processed blocks is cleared in the same pass (persistent gradient buffer, no fill launch).  Bit-identical to
   psdf_adamw_step over the whole tensor. */
int psdf_adamw_step_blocks(int64_t n_blocks, int block_elems, float* param, float* grad, float* exp_avg, float*
    exp_avg_sq, unsigned char* touched, unsigned char* active, float lr, float beta1, float beta2, float eps, int step,
    float grad_scale, int zero_grad, void* stream);
/* psdf_adamw_step_blocks for up to 8 tensors in ONE launch: host arrays [n_tensors] of block counts, block sizes, device pointers
   and per-tensor lr / beta1 / beta2 / eps / step (the lattices of a training step sit in different parameter groups). */
int psdf_adamw_step_blocks_multi(int n_tensors, const int64_t* n_blocks, const int* block_elems, float* const* params,
    float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs, unsigned char* const* touched,
    unsigned char* const* active, const float* lr, const float* beta1, const float* beta2, const float* eps, const int* step,
    float grad_scale, int zero_grad, void* stream);


/* ---- sampling.hip ---- */
/* replaces: OccupancyGrid::compute_grid_points / compute_random_sample_of_grid_points, src/OccupancyGrid.cu:88-117,179-208 */
int psdf_grid_points(int count, int nr_voxels_per_dim, float extent, const float* grid_translation, const int*
    voxel_indices, uint64_t rng_state, uint64_t rng_inc, int randomize, float* out_points, void* stream);

/* replaces: OccupancyGrid::update_with_density[_random_sample], src/OccupancyGrid.cu:368-420 */
int psdf_grid_update_with_density(int count, const int* voxel_indices, const float* density, float decay, float
    thresh, float* grid_values, uint8_t* grid_occupancy, void* stream);

/* replaces: OccupancyGrid::update_with_sdf[_random_sample], src/OccupancyGrid.cu:422-475 */
int psdf_grid_update_with_sdf(int count, const int* voxel_indices, const float* sdf, int nr_voxels_per_dim, float
    extent, const float* grid_translation, float inv_s, const float* inv_s_tensor, int full_update, float thresh,
    float* grid_values, uint8_t* grid_occupancy, void* stream);

/* replaces: OccupancyGrid::check_occupancy, src/OccupancyGrid.cu:339-365 */
int psdf_grid_check_occupancy(int count, int nr_voxels_per_dim, float extent, const float* grid_translation, const
    uint8_t* grid_occupancy, const float* points, uint8_t* out, void* stream);

/* replaces: the `weights` of run_net_sphere_traced (permuto_sdf_py/train_permuto_sdf.py:216-222: check_occupancy and
   check_point_inside_primitive of the traced end points, times the rays that met occupancy at all) and the
   compact_to_valid_samples behind it (src/RaySamplesPacked.cu:57-95).  A ray is valid iff no_hit [nr_rays] (1-byte bool) is 0,
   its point lies in an occupied voxel (the lookup of psdf_grid_check_occupancy, out of range = empty) and
   sqrtf((dx dx + dy dy) + dz dz) < sphere_radius for d = point - sphere_center (strict).  The valid rays are compacted IN RAY
   ORDER, without atomics: slot [nr_rays] int32 <- the dense row of a valid ray, -1 otherwise; pos, dirs_out [>= M, 3] <- points
   and dirs of the valid rays (rows from M on are not written); count [1] int32 <- M.  grid_translation, sphere_center: HOST
   pointers to 3 floats.  scratch: 2 * ceil(nr_rays / 256) int32.  nr_rays = 0 returns 0 without a launch; -1 for nr_rays < 0 or
   a NULL pointer. */
int psdf_trace_frame_select(int nr_rays, int nr_voxels_per_dim, float extent, const float* grid_translation, const uint8_t*
    grid_occupancy, float sphere_radius, const float* sphere_center, const float* points, const float* dirs, const uint8_t*
    no_hit, int* scratch, int* slot, float* pos, float* dirs_out, int* count, void* stream);

/* which form the last psdf_march_samples launched: 1 = march_kernel (a thread per ray), 2 = march_quad_kernel (four lanes per
   ray, unit grids with nr_rays <= 6144; PSDF_MARCH_FORM=thread|quad overrides); 0 = none yet.  Debug query (host only). */
int psdf_march_form(void);
/* replaces: OccupancyGrid::compute_samples_in_occupied_regions (src/OccupancyGrid.cu:212-257) and RaySampler::compute_samples_fg (src/RaySampler.cu:104-152);
   scratch: nr_rays * (3 + max_nr_samples_per_ray) 4-byte words */
int psdf_march_samples(int use_grid, int nr_rays, int nr_voxels_per_dim, float extent, const float* grid_translation,
    const uint8_t* grid_occupancy, const float* ray_origins, const float* ray_dirs, const float* ray_t_entry, const
    float* ray_t_exit, float min_dist_between_samples, int max_nr_samples_per_ray, int max_nr_samples, uint64_t
    rng_state, uint64_t rng_inc, int jitter, float* samples_pos, float* samples_dirs, float* samples_z, float*
    samples_dt, float* ray_fixed_dt, int* ray_start_end_idx, int* cur_nr_samples, int* scratch, const uint32_t*
    coarse_mask, void* stream);

/* replaces: OccupancyGrid::compute_first_sample_start_of_occupied_regions, src/OccupancyGrid.cu:259-300 */
int psdf_first_hit_samples(int nr_rays, int nr_voxels_per_dim, float extent, const float* grid_translation, const
    uint8_t* grid_occupancy, const float* ray_origins, const float* ray_dirs, const float* ray_t_entry, const float*
    ray_t_exit, int max_nr_samples, float* samples_pos, float* samples_dirs, float* samples_z, float* samples_dt,
    float* ray_fixed_dt, int* ray_start_end_idx, int* cur_nr_samples, int* scratch, const uint32_t* coarse_mask,
    void* stream);

/* replaces: OccupancyGrid::advance_sample_to_next_occupied_voxel, src/OccupancyGrid.cu:302-337 */
int psdf_advance_to_next_occupied_voxel(int count, int nr_voxels_per_dim, float extent, const float* grid_translation,
    const uint8_t* grid_occupancy, const float* samples_dirs, float* samples_pos, uint8_t* is_within_bounds, const
    uint32_t* coarse_mask, void* stream);

/* helper of the four marches above/below (no reference counterpart): "some voxel occupied" bit per 8x8x8 block of the
   Morton-ordered occupancy (kernels/permuto_sdf/OccupancyGridGPU.cuh:50-55 gives the order), psdf_occupancy_coarse_words(n)
   32-bit words; the marches copy it into LDS and answer the probes of empty blocks there (same results bit for bit).
   Optional everywhere: coarse_mask = NULL probes the bytes only.  Rebuild after every change of the occupancy. */
int psdf_occupancy_coarse_words(int nr_voxels_per_dim);
int psdf_occupancy_coarse_mask(int nr_voxels_per_dim, const uint8_t* grid_occupancy, uint32_t* coarse_mask, void*
    stream);

/* replaces: RaySampler::compute_samples_bg, src/RaySampler.cu:37-101 */
int psdf_samples_bg(int nr_rays, int nr_samples_per_ray, const float* ray_origins, const float* ray_dirs, const float*
    ray_t_exit, float sphere_radius, const float* sphere_center, uint64_t rng_state, uint64_t rng_inc, int randomize,
    int contract_3d_samples, float* samples_3d, float* samples_4d, float* samples_dirs, float* samples_z, float*
    samples_dt, float* ray_fixed_dt, int* ray_start_end_idx, void* stream);

/* replaces: Sphere::ray_intersection, src/Sphere.cu:42-79 */
int psdf_sphere_ray_intersection(int nr_rays, float radius, const float* center, const float* ray_origins, const
    float* ray_dirs, float* points_entry, float* t_entry, float* points_exit, float* t_exit, uint8_t* does_intersect,
    void* stream);

/* replaces: Sphere::rand_points_inside, src/Sphere.cu:82-108 */
int psdf_sphere_rand_points_inside(int count, float radius, const float* phi, const float* costheta, const float* u,
    float* points, void* stream);

/* replaces: RaySamplesPacked::compute_exact_nr_samples + compact_to_valid_samples, src/RaySamplesPacked.cu:44-95 */
int psdf_compact_offsets(int nr_rays, const int* ray_start_end_idx, int* scratch, int* total, void* stream);

/* replaces: RaySamplesPacked::compact_to_valid_samples, src/RaySamplesPacked.cu:57-95 */
int psdf_compact_copy(int nr_rays, const int* ray_start_end_idx, const int* offsets, const float* pos, const float*
    pos4, const float* dirs, const float* z, const float* dt, const float* sdf, const float* fixed_dt, float* o_pos,
    float* o_pos4, float* o_dirs, float* o_z, float* o_dt, float* o_sdf, float* o_fixed_dt, int* o_start_end, void*
    stream);

/* replaces: RaySamplesPacked::compute_per_sample_ray_idx, src/RaySamplesPacked.cu:124-146 */
int psdf_per_sample_ray_idx(int nr_rays, int nr_samples, const int* ray_start_end_idx, int* out, void* stream);

/* replaces: PermutoSDF::spherical_harmonics, src/PermutoSDF.cu:167-204 */
int psdf_spherical_harmonics(int count, int degree, const float* dirs, float* out, void* stream);

/* replaces: PermutoSDF::random_rays_from_reel, src/PermutoSDF.cu:67-112 */
int psdf_random_rays_from_reel(int nr_rays, int nr_images, int height, int width, const float* rgb_reel, const float*
    mask_reel, const float* K_reel, const float* tf_world_cam_reel, const int* pixel_indices, const int* img_indices,
    int has_mask, float* ray_origins, float* ray_dirs, float* gt_rgb, float* gt_mask, void* stream);

/* replaces: the Python loop of sphere_trace(), permuto_sdf_py/utils/sdf_utils.py:120-218 (first hit :127-133, per
   iteration step :167-185), with one slot per ray so that the loop is a fixed launch sequence (hipGraph) */
int psdf_first_hit_dense(int nr_rays, int nr_voxels_per_dim, float extent, const float* grid_translation, const
    uint8_t* grid_occupancy, const float* ray_origins, const float* ray_dirs, const float* ray_t_entry, const float*
    ray_t_exit, float* pos, uint8_t* converged, const uint32_t* coarse_mask, void* stream);
int psdf_sphere_trace_step(int count, int nr_voxels_per_dim, float extent, const float* grid_translation, const
    uint8_t* grid_occupancy, const float* dirs, const float* sdf, float sdf_multiplier, float sdf_converged_thresh,
    float* pts, uint8_t* converged, const uint32_t* coarse_mask, void* stream);
/* the same iteration with the long marches compacted into a second, densely packed launch (same results): work_flags
   [count] bytes, work_list [count] ints, work_count [1] int that the caller has zeroed; coarse_mask optional (the marches) */
int psdf_sphere_trace_step_compacted(int count, int nr_voxels_per_dim, float extent, const float* grid_translation, const
    uint8_t* grid_occupancy, const float* dirs, const float* sdf, float sdf_multiplier, float sdf_converged_thresh,
    float* pts, uint8_t* converged, uint8_t* work_flags, int* work_list, int* work_count, const uint32_t* coarse_mask,
    void* stream);

/* ---- volume_rendering.hip ---- */
/* replaces: (helper) replaces the atomicAdd slot counters, e.g. kernels/permuto_sdf/OccupancyGridGPU.cuh:599 */
int psdf_exclusive_scan_i32(int n, const int* in, int* out, int* total, void* stream);

/* replaces: VolumeRendering::cumprod_alpha2transmittance, src/VolumeRendering.cu:169-201 */
int psdf_cumprod_alpha2transmittance(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples,
    const float* alpha, float* transmittance, float* bg_transmittance, void* stream);

/* replaces: VolumeRendering::cumprod_alpha2transmittance_backward, src/VolumeRendering.cu:530-564 */
int psdf_cumprod_alpha2transmittance_backward(int nr_rays, const int* start_end, int equal, int fixed, int
    max_nr_samples, const float* grad_bg, const float* alpha, const float* bg, const float* cumsumLV, float*
    grad_alpha, void* stream);

/* replaces: VolumeRendering::integrate_with_weights, src/VolumeRendering.cu:204-232 */
int psdf_integrate_with_weights(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const
    float* rgb, const float* weights, float* pred, void* stream);

/* replaces: VolumeRendering::integrate_with_weights_backward, src/VolumeRendering.cu:567-601 */
int psdf_integrate_with_weights_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples,
    const float* grad_pred, const float* rgb, const float* weights, float* grad_rgb, float* grad_weights, int
    reference_compat, void* stream);

/* replaces: VolumeRendering::sum_over_each_ray, src/VolumeRendering.cu:272-344 */
int psdf_sum_over_each_ray(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int channels,
    const float* values, float* sum_per_ray, float* sum_per_sample, void* stream);

/* replaces: VolumeRendering::sum_over_each_ray_backward, src/VolumeRendering.cu:604-668 */
int psdf_sum_over_each_ray_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int
    channels, const float* grad_per_ray, const float* grad_per_sample, float* grad_values, void* stream);

/* replaces: VolumeRendering::cumsum_over_each_ray (:346-376) and compute_cdf (:379-408) */
int psdf_cumsum_over_each_ray(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const
    float* values, int inverse, int exclusive, float* out, void* stream);

/* replaces: VolumeRendering::sdf2alpha, src/VolumeRendering.cu:234-269 */
int psdf_sdf2alpha(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float*
    ray_fixed_dt, const float* samples_dt, const float* sdf, float inv_s, int dynamic_inv_s, float inv_s_multiplier,
    float* alpha, void* stream);
/* sdf2alpha -> clip(0,1) -> 1 - alpha + 1e-7 -> cumprod_alpha2transmittance -> alpha * T -> sum_over_each_ray -> / clamp(sum, 1e-6)
   -> compute_cdf in ONE launch: the operator chain of importance_sampling_sdf_model (permuto_sdf_py/utils/sdf_utils.py:383-423),
   bit-identical to calling the operators one by one; cdf [M,1] (zero-filled by the caller where slots belong to no ray) */
int psdf_sdf_importance_cdf(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* ray_fixed_dt,
                            const float* samples_dt, const float* sdf, float inv_s, int dynamic_inv_s, float inv_s_multiplier,
                            float* cdf, void* stream);

/* replaces: VolumeRendering::compute_dt, src/VolumeRendering.cu:135-167 */
int psdf_compute_dt(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float*
    samples_z, const float* ray_t_exit, int use_ray_t_exit, float* dt, void* stream);

/* replaces: VolumeRendering::volume_render_nerf, src/VolumeRendering.cu:40-83 */
int psdf_volume_render_nerf(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float*
    rgb, const float* density, const float* samples_z, const float* samples_dt, float* pred_rgb, float* pred_depth,
    float* bg_transmittance, float* weight_per_sample, void* stream);

/* replaces: VolumeRendering::volume_render_nerf_backward, src/VolumeRendering.cu:86-132 */
int psdf_volume_render_nerf_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples,
    const float* grad_pred_rgb, const float* grad_bg_transmittance, const float* pred_rgb, const float*
    bg_transmittance, const float* rgb, const float* density, const float* samples_dt, float* grad_rgb, float*
    grad_density, void* stream);

/* replaces: VolumeRendering::importance_sample, src/VolumeRendering.cu:410-461 */
int psdf_importance_sample(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float*
    ray_origins, const float* ray_dirs, const float* ray_fixed_dt, const float* samples_z, const float* cdf, int
    nr_importance_samples, uint64_t rng_state, uint64_t rng_inc, int jitter, float* out_pos, float* out_dirs, float*
    out_z, void* stream);

/* replaces: VolumeRendering::combine_uniform_samples_with_imp, src/VolumeRendering.cu:464-525 */
int psdf_combine_uniform_samples_with_imp(int nr_rays, const int* uni_start_end, int uni_equal, int uni_fixed, int
    uni_max_nr_samples, const float* ray_origins, const float* ray_dirs, const float* ray_t_exit, const float*
    uni_fixed_dt, const float* uni_z, const float* uni_sdf, int has_sdf, int nr_imp, const float* imp_z, const float*
    imp_sdf, int out_max_nr_samples, float* out_pos, float* out_dirs, float* out_z, float* out_dt, float* out_sdf,
    float* out_fixed_dt, int* out_start_end, int* out_cur_nr_samples, int* scratch, void* stream);

/* ---- mesh.hip ---- */
/* replaces: the host side of extract_mesh_from_sdf_model (permuto_sdf_py/utils/sdf_utils.py:252-292: the n^3 volume assembled in
   host memory, then skimage.measure.marching_cubes) by marching tetrahedra on the device, streamed over slabs of x-planes.  The
   triangulation, the inside test (vol - level < 0 in fp32), the welding by grid edge and the vertex order are those of
   compat/skimage/measure.py; the tables and the winding rule are csrc/mesh_tables.h.
   Layout shared by the three passes: the volume is [X, Y, Z] fp32 with Z fastest; the per-point buffers vol / valid / mask / vincl
   hold `nplanes` consecutive x-planes starting at global plane `xbase` (xbase + nplanes <= X).  `valid` (bytes, NULL = all): points
   that carry a value; an edge needs two valid ends, a cell eight valid corners, other values are never read.
   psdf_mesh_classify: vertex planes [p0, p1) -> mask (7 bits: owned crossing edges in the directions z, y, yz, x, xz, xy, xyz;
   written at the buffer's slots) and vcount [(p1 - p0) Y Z] int32 = popcount(mask); value planes p0 .. min(p1, X - 1) must be in the
   buffer.  Cell planes [c0, c1), c1 <= X - 1 -> tcount [(c1 - c0) Y Z] int32 triangles per cell (indexed like points; 0 on the
   last row / column); value planes c0 .. c1 must be in the buffer.  Either range may be empty.
   The caller scans both counts INCLUSIVELY (no scan here: nothing allocates) and stores, at the buffer's slots, vincl = scan of
   vcount + number of vertices of earlier slabs; tincl = scan of tcount stays local to the range. */
int psdf_mesh_classify(const float* vol, const uint8_t* valid, float level, int X, int Y, int Z, int xbase, int nplanes, int p0,
    int p1, int c0, int c1, uint8_t* mask, int32_t* vcount, int32_t* tcount, void* stream);
/* vertices of the edges owned by planes [p0, p1), at row (global id - v_off) of verts [., 3] (index coordinates, fp32:
   t = f_lo / (f_lo - f_hi), p = p_lo + (p_hi - p_lo) t), edges [., 2] int64 (optional: linear indices (x Y + y) Z + z of the two
   ends, lo first) and normals [., 3] (optional; -2 unless the buffer holds the whole volume: the stand-in's normal, np.gradient of
   the volume at both ends interpolated with t, normalised, negated) */
int psdf_mesh_emit_vertices(const float* vol, float level, int X, int Y, int Z, int xbase, int nplanes, int p0, int p1, const
    uint8_t* mask, const int32_t* vincl, int64_t v_off, float* verts, int64_t* edges, float* normals, void* stream);
/* triangles of cell planes [c0, c1) as global vertex ids, at rows tincl - count of faces [., 3] int32, ordered by (cell,
   tetrahedron, triangle); mask / vincl of vertex planes c0 .. c1 must be in the buffer */
int psdf_mesh_emit_faces(const float* vol, const uint8_t* valid, float level, int X, int Y, int Z, int xbase, int nplanes, int c0,
    int c1, const uint8_t* mask, const int32_t* vincl, const int32_t* tincl, int32_t* faces, void* stream);
/* replaces: the torch.meshgrid + chunk loop of sdf_utils.py:262-276.  points [count, 3] of the linear indices first .. first +
   count - 1 (relative to plane x0, Z fastest) of the grid with axis coordinates xs [nx], ys [Y], zs [Z] (the caller's
   torch.linspace, bit for bit) */
int psdf_mesh_grid_points(int nx, int Y, int Z, int x0, int64_t first, int64_t count, const float* xs, const float* ys, const
    float* zs, float* points, void* stream);
/* sparse extraction: valid[i] = 1 iff one of the 27 probes points[i] + {-h, 0, h}^3 lies in an occupied voxel of the Morton-ordered
   occupancy grid (h = mesh spacing <= voxel size: then every corner of a cell that contains a surface point of an occupied voxel is
   valid); skip[i] = !valid[i] (optional: the mask the masked encode / MLP launches take) */
int psdf_mesh_sparse_mask(int64_t count, int nr_voxels_per_dim, float extent, const float* grid_translation, const uint8_t*
    grid_occupancy, const float* points, float h, uint8_t* valid, uint8_t* skip, void* stream);

/* ---- mesh_eval.hip ---- */
/* The DTU Chamfer protocol the reference scores its meshes with (permuto_sdf_py/experiments/evaluation/
   evaluate_chamfer_distance.py calls permuto_sdf_py/experiments/evaluation/DTUeval-python/eval.py) on device tensors.  The
   entries allocate nothing and never synchronise; sorts and scans are the caller's; an empty batch returns 0 before any
   pointer check.  The uniform grid of a cloud is (origin_edge [4] = lower corner and cell edge, dims [3]), host arrays, from
   psdf_mesh_eval_grid_plan (csrc/mesh_eval_plan.h). */
/* reference points per LDS tile of psdf_mesh_nn_cooperative (host only) */
int psdf_mesh_eval_tile_capacity(void);
/* host only: the grid of n_points points with bounding box [lo, hi] (3 doubles each; the finite points' fp32 extremes), a cell
   edge >= min_edge (the caller's search radius, 0: none) and at most cell_budget cells (<= 0: the default) -> origin_edge [4],
   dims [3], *cells = dims[0] dims[1] dims[2] (int64), *query_blocks (optional) = blocks of 4 x 4 x 4 cells.  -1: bad box / count;
   -2: more than 2^31 - 1 points */
int psdf_mesh_eval_grid_plan(const double* lo, const double* hi, int64_t n_points, double min_edge, int64_t cell_budget, float*
    origin_edge, int* dims, int64_t* cells, int64_t* query_blocks);
/* replaces: the lattice sampling of every triangle, eval.py:9-18 (sample_single_tri) and :53-69 (edge vectors, the spacing
   thr = density sqrt(l1 l2 / area2), n = floor(l / thr), one pool task per triangle).  V [nV, 3] fp32, F [nF, 3] int32;
   counts [nF] int32 <- samples of every triangle: decisions in float64 from the fp32 corners, (i + 1/2) / max(n, 1e-7) and the
   strict a + b < 1 as written there; a triangle of zero area counts 0.  *overflow (int32, zeroed by the caller) |= 1 when a
   triangle has more than 30 000 lattice steps on an edge, |= 2 when a face names a vertex outside [0, nV): both count 0. */
int psdf_mesh_sample_count(const float* V, int64_t nV, const int32_t* F, int64_t nF, double density, int32_t* counts, int32_t*
    overflow, void* stream);
/* incl [nF] int64 = the caller's INCLUSIVE scan of counts; samples [incl[nF - 1], 3] fp32 <- p0 + a e1 + b e2 evaluated in
   float64 and rounded once, triangle by triangle, i-major, j-minor (the order of eval.py:67-69) */
int psdf_mesh_sample_emit(const float* V, int64_t nV, const int32_t* F, int64_t nF, double density, const int64_t* incl, float*
    samples, void* stream);
/* keys [n] int32 <- the cell of every point (block_log2 = 0: (cx ny + cy) nz + cz) or its block of (1 << block_log2)^3 cells
   (numbered the same way over the blocks); cx = (int)clamp((p - origin) / edge, 0, n - 1) with the clamp in fp32: the one cell
   function of this file.  A point with a non-finite coordinate gets the number of cells (blocks): the key past every cell. */
int psdf_mesh_eval_cell_keys(const float* points, int64_t n, const float* origin_edge, const int* dims, int block_log2, int32_t*
    keys, void* stream);
/* start [cells + 1] int32 <- first position of sorted_keys [n] (ascending: the caller's sort) with a key >= c: cell c owns
   [start[c], start[c + 1]) and start[cells] = number of finite points.  n = 0 is a valid call (all zero). */
int psdf_mesh_eval_cell_ranges(const int32_t* sorted_keys, int64_t n, int64_t cells, int32_t* start, void* stream);
/* replaces: the radius_neighbors query and the sequential kill loop of eval.py:85-93 (after the shuffle of :80-81) by sweeps of
   the parallel form of the same set (the lexicographically first maximal independent set of the d <= radius graph under the
   order `rank`).  points [n, 3] / rank [n] / keys [n] in CELL-SORTED order, cell_start from psdf_mesh_eval_cell_ranges of a
   grid with edge >= radius (1 + 1/512) (-1 otherwise); state [n] bytes, zeroed by the caller before the first sweep: 0
   undecided, 1 kept, 2 dropped.  One call = one in-place sweep; *undecided (int32, zeroed by the caller before every sweep) +=
   points still undecided after it.  The caller sweeps until it reads 0; d = sqrtf of the fp32 difference form. */
int psdf_mesh_thin_sweep(const float* points, const int32_t* rank, const int32_t* keys, int64_t n, const int32_t* cell_start,
    const float* origin_edge, const int* dims, float radius, uint8_t* state, int32_t* undecided, void* stream);
/* replaces: the KD-tree kneighbors queries of eval.py:118-121 and :131-133 (data -> scan, scan -> data, distances below
   max_dist averaged).  refs [nr, 3] sorted by cell with cell_start; queries [nq, 3] sorted by block of 4 x 4 x 4 cells of THE
   SAME grid (psdf_mesh_eval_cell_keys with block_log2 = 2) with query_block_start [blocks + 1].  One workgroup per block stages
   the references of the block and its one-cell halo through LDS tiles and every lane tests its query: dist [nq] / idx [nq]
   (position in the SORTED references) <- nearest reference strictly closer than max_dist, else (max_dist, -1); open [nq] <- 1
   where that is not yet proven (best > distance to the boundary of the cells searched); *nr_open (int32, zeroed by the caller)
   += their number.  Queries outside every block (non-finite ones) are not written: the caller pre-fills (max_dist, -1, 0). */
int psdf_mesh_nn_cooperative(const float* queries, int64_t nq, const int32_t* query_block_start, const float* refs, int64_t nr,
    const int32_t* cell_start, const float* origin_edge, const int* dims, float max_dist, float* dist, int32_t* idx, uint8_t*
    open, int32_t* nr_open, void* stream);
/* finishes the queries with open != 0: shells of cells around the query's own cell, from shell 2 on, until best <= distance to
   the boundary of the shells searched (best starts at max_dist: never further than the cut-off) */
int psdf_mesh_nn_ring(const float* queries, int64_t nq, const float* refs, int64_t nr, const int32_t* cell_start, const float*
    origin_edge, const int* dims, float max_dist, float* dist, int32_t* idx, const uint8_t* open, void* stream);

/* ---- mesh_clean.hip ---- */
/* What the reference does to an extracted mesh before it scores it, on device tensors: the box cull of
   permuto_sdf_py/experiments/evaluation/create_my_meshes.py:72-75 and, for scenes trained without masks, the mask cull, face
   filter and largest component of permuto_sdf_py/experiments/evaluation/evaluate_chamfer_distance.py:110-167.  The entries
   allocate nothing and never synchronise; sorts and scans are the caller's; an empty batch returns 0 before any pointer check.
   Two rules are restated from their libraries' published behaviour and are UNPINNED here (neither library is available to the
   tests): the row spans of OpenCV's MORPH_ELLIPSE (the caller passes them in) and trimesh's face adjacency (an edge links two
   faces iff it occurs in exactly two half-edges).  *flag (int32, zeroed by the caller): |= 2 a face names a vertex outside
   [0, nV); |= 4 a union-find loop exceeded its cap (psdf_mesh_clean_union_find_cap). */
/* host only: the launch plan of the dilation (csrc/mesh_clean_plan.h) for n views of H x W and an element whose row k has the
   half-width half_widths[k] (count rows, odd) -> out [PSDF_MESH_CLEAN_PLAN_FIELDS] int64: 0 the radius r = count / 2; 1 output
   rows per workgroup; 2 rows staged in LDS (field 1 + 2 r); 3, 4 tiles along x and y; 5 packed words per row, ceil(W / 32); 6
   workgroups of psdf_mesh_clean_dilate; 7 workgroups of psdf_mesh_clean_row_distance; 8 bytes of LDS of a dilation workgroup.
   -1: n < 0, H or W < 1, an even or empty element, a half-width outside [0, 254]; -2: more than 255 rows, or more than 2^31 - 1
   workgroups */
#define PSDF_MESH_CLEAN_PLAN_FIELDS 9
int psdf_mesh_clean_dilate_plan(int64_t n, int64_t H, int64_t W, const int* half_widths, int64_t count, int64_t* out);
/* host only: the iteration cap of the union-find loops over n nodes, n + 1 */
int64_t psdf_mesh_clean_union_find_cap(int64_t n);
/* replaces: the threshold `> 128` of evaluate_chamfer_distance.py:135 (moved before the dilation: dilating and thresholding
   commute for a flat element) and the horizontal half of cv.dilate (:134).  masks [n, H, W] uint8; hd [n, H, W] uint8 <-
   distance along the row to the nearest pixel with value > threshold, 255 when that is 255 or more or the row has none */
int psdf_mesh_clean_row_distance(const uint8_t* masks, int64_t n, int H, int W, int threshold, uint8_t* hd, void* stream);
/* replaces: cv.getStructuringElement(cv.MORPH_ELLIPSE, (101, 101)) and cv.dilate, evaluate_chamfer_distance.py:133-134, for any
   element made of centred row spans.  half_widths [count]: a HOST array; words [n, H, ceil(W / 32)] int32 <- the dilated masks,
   pixel (y, x) at bit x & 31 of word x >> 5, padding bits 0: set iff hd[y + dy, x] <= half_widths[dy + r] for a dy with y + dy
   inside the image (nothing is set outside it: cv.dilate's default border) */
int psdf_mesh_clean_dilate(const uint8_t* hd, int64_t n, int H, int W, const int* half_widths, int count, int32_t* words, void*
    stream);
/* replaces: clean_points_by_mask, evaluate_chamfer_distance.py:110-143 (the projection of :130-132, the ones-padded image and the
   clipped lookup of :137-140, the AND of :142).  V [nV, 3] fp32; world_mats [views, 12] float64: the first three rows of every
   world_mat_i; keep [nV] bytes <- 1 iff every view keeps the vertex: p = ((P0 x + P1 y) + P2 z) + P3 per row in float64, u = p0 /
   p2, v = p1 / p2 rounded half to even; with 0 <= u < W and 0 <= v < H the view keeps it iff bit (v, u) of its words is set,
   otherwise -- and for a non-finite u or v -- it keeps it.  No test of the sign of p2: the reference has none. */
int psdf_mesh_clean_inside_masks(const float* V, int64_t nV, const double* world_mats, int views, const int32_t* words, int H, int
    W, uint8_t* keep, void* stream);
/* replaces: faces_mask of evaluate_chamfer_distance.py:151.  face_keep [nF] bytes <- 1 iff keep [nV] is set for the face's three
   vertices (and face_mask [nF], optional, for the face); a face out of range raises the flag and is dropped */
int psdf_mesh_clean_face_keep(const int32_t* F, int64_t nF, const uint8_t* keep, int64_t nV, const uint8_t* face_mask, uint8_t*
    face_keep, int32_t* flag, void* stream);
/* replaces: indexes and new_vertices of evaluate_chamfer_distance.py:147-149 and :156 (remove_marked_vertices(mask, True) for
   the box cull).  incl [nV] int32: the caller's INCLUSIVE scan of keep; a kept vertex moves to row incl - 1 of V_out (NV_out
   [.., 3] fp32 and edges_out [.., 2] int64 where NV / edges are given); vertex_map [nV] int32 <- the new row, -1 where removed */
int psdf_mesh_clean_emit_vertices(int64_t nV, const uint8_t* keep, const int32_t* incl, const float* V, const float* NV, const
    int64_t* edges, float* V_out, float* NV_out, int64_t* edges_out, int32_t* vertex_map, void* stream);
/* replaces: new_faces of evaluate_chamfer_distance.py:152-155.  incl [nF] int32: the caller's inclusive scan of face_keep; a kept
   face moves to row incl - 1 of F_out, renumbered through vertex_map */
int psdf_mesh_clean_emit_faces(const int32_t* F, int64_t nF, const uint8_t* face_keep, const int32_t* incl, const int32_t*
    vertex_map, int32_t* F_out, void* stream);
/* replaces: the edge matching inside trimesh's Trimesh.split(only_watertight=False), evaluate_chamfer_distance.py:160
   (face_adjacency: rows of the sorted edges that occur exactly twice).  keys [3 nF] int64 <- (min << 32) | max of the half-edge
   e of face f at slot 3 f + e */
int psdf_mesh_clean_edge_keys(const int32_t* F, int64_t nF, int64_t nV, int64_t* keys, int32_t* flag, void* stream);
/* sorted_keys [3 nF] ascending and slot [3 nF] int64, the slot each key came from (the caller's stable sort): unites the two
   faces slot / 3 of every run of exactly two equal keys whose endpoints differ.  parent [nF] int32: the caller's 0 .. nF - 1;
   the larger root is hooked under the smaller by compare-and-swap, so parent[i] <= i throughout */
int psdf_mesh_clean_link_edges(const int64_t* sorted_keys, const int64_t* slot, int64_t nF, int32_t* parent, int32_t* flag, void*
    stream);
/* vertex connectivity: unites the three vertices of every face in parent [nV] (the caller's 0 .. nV - 1) */
int psdf_mesh_clean_link_vertices(const int32_t* F, int64_t nF, int64_t nV, int32_t* parent, int32_t* flag, void* stream);
/* replaces: the connected-components labelling of Trimesh.split.  labels [n] int32 <- the root of every node, the smallest index
   of its component; sizes [n] int32 (optional, zeroed by the caller) += 1 at every node's label */
int psdf_mesh_clean_flatten(int32_t* parent, int64_t n, int32_t* labels, int32_t* sizes, int32_t* flag, void* stream);
/* vertex connectivity: vertex_label [nV] from psdf_mesh_clean_flatten; first_face [nV] int32 (filled with INT32_MAX by the
   caller) <- the smallest face of every vertex component; labels [nF] <- that face for every face; sizes [nF] (zeroed) += 1 */
int psdf_mesh_clean_face_labels(const int32_t* F, int64_t nF, int64_t nV, const int32_t* vertex_label, int32_t* first_face,
    int32_t* labels, int32_t* sizes, void* stream);

/* ---- image_eval.hip ---- */
/* The image scores of the reference's held-out views (permuto_sdf_py/experiments/evaluation/evaluate_psnr.py: piq.psnr and
   piq.ssim on both images times the mask) on device tensors, accumulated in float64 without floating-point atomics: the same
   input gives the same bits on every run.  An image is a logical (N, C, H, W) tensor read in place: `x` a device pointer to its
   first element, `x_u8` 0: fp32 elements, 1: uint8 elements (v stands for v / 255.0), `x_strides` a HOST array of the four
   element strides (>= 0; an NHWC buffer viewed as NCHW is read without a copy).  pred and gt may differ in element type and
   strides.  mask: NULL, or a logical (N, 1, H, W) tensor given the same way (its channel stride is not read); it multiplies both
   images, data_range (> 0) divides both, in double.  The entries allocate nothing and never synchronise; N = 0 returns 0 before
   any pointer check. */
/* host only: the launch plan of psdf_image_ssim (csrc/image_eval_plan.h) -> out [PSDF_IMAGE_EVAL_PLAN_FIELDS] int64:
   0 the pooling factor f = max(1, round_half_even(min(H, W) / 256)) (1 when downsample = 0); 1, 2 the pooled extents H / f,
   W / f; 3, 4 the extents of the map, pooled - kernel_size + 1; 5, 6 the map entries per workgroup tile (rows, columns); 7, 8 the
   tiles along the map's rows and columns; 9 bytes of psdf_image_ssim's workspace; 10 partial sums per image of
   psdf_image_sq_diff; 11 bytes of its workspace; 12 the largest kernel_size; 13 bytes of LDS of an SSIM workgroup.
   -1: N < 0, an extent < 1, kernel_size even, < 1 or above out[12], or a pooled side shorter than kernel_size; -2: more than
   2^31 - 1 workgroups */
#define PSDF_IMAGE_EVAL_PLAN_FIELDS 14
int psdf_image_eval_plan(int64_t N, int C, int H, int W, int kernel_size, int downsample, int64_t* out);
/* host only: partial sums per image of psdf_image_sq_diff, ceil(H W / 2048) (-1: an extent < 1) -- the one plan value an image
   smaller than the SSIM window still has */
int64_t psdf_image_sq_diff_partials(int H, int W);
/* replaces: the sum inside piq.psnr's mean squared error.  out [N] float64 <- sum over (c, h, w) of (pred - gt)^2 of the masked,
   range-divided values; workspace [N * psdf_image_sq_diff_partials(H, W)] float64: one partial per workgroup, written in a fixed
   order and added in a fixed order by a finishing launch */
int psdf_image_sq_diff(const void* pred, int pred_u8, const int64_t* pred_strides, const void* gt, int gt_u8, const int64_t*
    gt_strides, const void* mask, int mask_u8, const int64_t* mask_strides, int64_t N, int C, int H, int W, double data_range,
    double* workspace, double* out, void* stream);
/* replaces: piq.ssim (average pooling by f with floor mode, the kernel_size x kernel_size Gaussian window of kernel_sigma over
   valid positions only, c1 = k1^2, c2 = k2^2, mean over the map and then over channels).  One fused pass per (image, channel,
   tile): pooled values, the horizontally filtered moments and the reduction live in LDS only.  out [N] float64 <- the score of
   every image; map: NULL, or [N, C, out[3], out[4]] float64 <- the map itself; workspace: out[9] bytes.  -1 also for a
   non-positive kernel_sigma or data_range and a NULL image, workspace or out */
int psdf_image_ssim(const void* pred, int pred_u8, const int64_t* pred_strides, const void* gt, int gt_u8, const int64_t*
    gt_strides, const void* mask, int mask_u8, const int64_t* mask_strides, int64_t N, int C, int H, int W, double data_range,
    int kernel_size, double kernel_sigma, double k1, double k2, int downsample, double* workspace, double* out, double* map,
    void* stream);

/* ---- nerf_render.hip ---- */
/* NeRF training of a foreground (permuto_sdf_py/train_nerf.py): the rendering of a packed container with all three per-ray
   outputs and their gradients, the loss tail, and the glue between NerfHash's two nets.  The entries allocate nothing and never
   synchronise; a count <= 0 returns 0 before any pointer is looked at. */
/* host only: the launch plan (csrc/nerf_render_plan.h) -> out [PSDF_NERF_RENDER_PLAN_FIELDS] int64: 0 workgroups of the loss
   kernel (= partial sums per term), 1 bytes of psdf_nerf_loss's workspace, 2 rays one pass of the full loss grid covers, 3 the
   register chunks K of 64 samples psdf_nerf_render_backward holds for max_per_ray (1, 2 or 4).
   -1: nr_rays < 0, max_per_ray < 1, out NULL; -2: nr_rays > (2^31 - 1) / 3, max_per_ray > 256 */
#define PSDF_NERF_RENDER_PLAN_FIELDS 4
int psdf_nerf_render_plan(int64_t nr_rays, int max_per_ray, int64_t* out);
/* replaces: NerfHash's softplus (models.py:517), VolumeRenderingNerf.compute_weights + integrate (volume_rendering_modules.py:
   72-86,176-190) as train_nerf.py:70-71 calls them for the FOREGROUND.  Ray-index arguments, raw_density [M], dt [M], rgb [M,3]
   as psdf_nerf_composite_forward.  pred [R,3] <- sum w rgb (the sweep and the summation order of psdf_nerf_composite_forward:
   the same bits as its pred_bg), weights_sum [R] <- sum w, bg_transmittance [R] <- T of the ray's last sample; each output may
   be NULL on its own (rgb may be NULL when pred is).  Empty and overflowed rays: 0, 0 and 1.  Any ray length.
   -1: every output NULL, or a NULL input that is needed */
int psdf_nerf_render_forward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float*
    raw_density, const float* dt, const float* rgb, float* pred, float* weights_sum, float* bg_transmittance, void* stream);
/* Backward of the above for upstream grad_pred [R,3], grad_weights_sum [R], grad_bg_transmittance [R]: each may be NULL (= no
   gradient arrives there), at least one is given.  grad_raw_density [M]; grad_rgb [M,3] optional (zeros without grad_pred).
   The weight gradient of a sample is <grad_pred, rgb> + grad_weights_sum; max_per_ray and reference_compat as in
   psdf_nerf_composite_backward: a ray longer than declared gets NaN in every gradient, max_per_ray > 256 -> -2.  Samples of
   rays the reference skips (empty, overflowed) are not written: zero-fill the outputs when the container can hold such rays. */
int psdf_nerf_render_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int max_per_ray,
    const float* grad_pred, const float* grad_weights_sum, const float* grad_bg_transmittance, const float* raw_density, const
    float* dt, const float* rgb, int reference_compat, float* grad_raw_density, float* grad_rgb, void* stream);
/* replaces: train_nerf.py:203-207 and torch autograd of it.  pred, gt [R,3]; hit: uint8 [R] or NULL (= 1).  terms [2] (device)
   <- 0: mean over 3 R of (gt - pred)^2 hit[ray];  1: mean over R of BCE(clip(weights_sum, 1e-3, 1 - 1e-3), gt_mask), computed
   when weights_sum and gt_mask [R] are given (both or neither), else 0.  loss [1] (optional) <- loss + terms[0] + mask_weight
   terms[1] (the reference's mask_weight: 0.1).  grad_pred [R,3] (optional) and grad_weights_sum [R] (optional) <- the gradient
   of that sum; grad_weights_sum is 0 where the clip is active (a value AT a bound passes, as in torch.clamp) and without the
   mask term.  workspace: out[1] bytes of psdf_nerf_render_plan.  No floating-point atomics: partial sums per workgroup of a
   fixed grid, added in double in a fixed order by a finishing launch -- the same inputs give the same bits on every call.
   -1 also for a NaN mask_weight; -2 for nr_rays > (2^31 - 1) / 3 */
int psdf_nerf_loss(int64_t nr_rays, const float* pred, const float* gt, const unsigned char* hit, const float* weights_sum,
    const float* gt_mask, float mask_weight, double* workspace, float* terms, float* loss, float* grad_pred, float*
    grad_weights_sum, void* stream);
/* replaces: between NerfHash's two nets (models.py:509-513) gelu + t() + cat.  fd [65, M] the density net's feature-major
   output (row 0: the raw density), sh [M, 16] from psdf_spherical_harmonics (degree 4) -> x2 [80, M] = [gelu(fd[1:65]); sh^T],
   one launch.  -1: M < 0 or a NULL pointer; -2: M >= 2^31 */
int psdf_nerf_head_join(int64_t M, const float* fd, const float* sh, float* x2, void* stream);
/* replaces: gelu_backward + cat of the same place's backward.  grad_raw [M] (the density's gradient), dX2 [>= 64, M] (row
   stride M: the colour head's input gradient, its first 64 rows are read), fd [65, M] -> grad_fd [65, M] = [grad_raw;
   dX2[:64] * gelu'(fd[1:65])] */
int psdf_nerf_head_join_backward(int64_t M, const float* grad_raw, const float* dX2, const float* fd, float* grad_fd, void*
    stream);

/* ---- sdf_fit.hip ---- */
/* Fitting the SDF network to an oriented point cloud (permuto_sdf_py/train_sdf_from_mesh.py, train_4d_sdf.py): the batch of a
   step and the loss tail.  P is the dimension of a position: 3, or 4 with time as the last column.  n_surf rows on the surface
   come first, n_off rows off it follow; N = n_surf + n_off.  The entries allocate nothing and never synchronise; N = 0 returns 0
   before any pointer is looked at; -1 for a negative count, another P, a NULL pointer that is needed; -2 for a count beyond
   2^31 - 1. */
/* host only: the launch plan (csrc/sdf_fit_plan.h) -> out [PSDF_SDF_FIT_PLAN_FIELDS] int64: 0 workgroups of the loss kernel
   (= partial sums per term), 1 bytes of psdf_sdf_fit_loss's workspace, 2 rows one pass of the full loss grid covers, 3
   workgroups of the batch kernel */
#define PSDF_SDF_FIT_PLAN_FIELDS 4
int psdf_sdf_fit_plan(int64_t n_surf, int64_t n_off, int64_t* out);
/* replaces: the batch of train_sdf_from_mesh.py:118-123 and train_4d_sdf.py:200-208 (randint, index_select of points and
   normals, rand_points_inside, rand, two cat), the random numbers coming from the caller (torch's generator).  points [N, P]:
   rows r < n_surf <- cloud_points [M, P] row indices[r], the others <- lo[c] + uniforms[r - n_surf, c] * (hi[c] - lo[c]), one
   rounding per operation; normals [n_surf, 3] <- cloud_normals [M, 3] row indices[r].  lo, hi: HOST arrays of P floats.
   indices: int64 on the device.  AN INDEX IS CLAMPED TO [0, M - 1]: no index can make the kernel read outside the cloud.
   -1 also for M < 1 with n_surf > 0 */
int psdf_sdf_fit_batch(int P, int64_t M, int64_t n_surf, int64_t n_off, const float* cloud_points, const float* cloud_normals,
    const int64_t* indices, const float* uniforms, const float* lo, const float* hi, float* points, float* normals, void*
    stream);
/* replaces: sdf_loss, permuto_sdf_py/utils/sdf_utils.py:16-57, the division by 30000 behind it (train_sdf_from_mesh.py:136) and
   torch autograd of both.  sdf [N], gradients [N, P] (g: the first three columns, train_4d_sdf.py:213), normals [n_surf, 3];
   weights: HOST array of 4 floats (the reference's 5e1, 1e2, 3e3, 1e2).  terms [4] (device) <- the unweighted means
     0 over N:       w | |g| - 1 |, w = exp(-s^2 / (2 eik_clamp^2)) for eik_clamp > 0, else 1; w is not differentiated
     1 over n_surf:  1 - g . n / (max(|g|, 1e-8) max(|n|, 1e-8))      (F.cosine_similarity)
     2 over n_surf:  |s|
     3 over n_off:   exp(-sharpness |s|)
   with sign(0) = 0, the gradient of |g| at 0 equal to 0, the clamps of term 1 acting on the norms' values only (their
   derivatives stay those of the norms, as in torch), and 0 for a mean over no rows.  loss [1] (optional) <- loss +
   scale * sum_k weights[k] terms[k].  grad_sdf [N], grad_gradients [N, P] (both or none) <- the gradient of that sum; the time
   column of grad_gradients is written as 0.  workspace: out[1] bytes of psdf_sdf_fit_plan.  No floating-point atomics: partial
   sums per workgroup of a fixed grid, added in double in a fixed order by a finishing launch -- the same inputs give the same
   bits on every call.  -1 also for a NaN weight, sharpness, eik_clamp or scale */
int psdf_sdf_fit_loss(int P, int64_t n_surf, int64_t n_off, const float* sdf, const float* gradients, const float* normals,
    const float* weights, float sharpness, float eik_clamp, float scale, double* workspace, float* terms, float* loss, float*
    grad_sdf, float* grad_gradients, void* stream);

/* ---- frame_trace.hip ---- */
/* replaces: what run_net_sphere_traced does after the networks (permuto_sdf_py/train_permuto_sdf.py:224-242: the integrals of
   colour and SDF gradient with one sample per ray and a weight in {0, 1}, F.normalize, the weight sum, lin2nchw) and
   rotate_normals_to_cam_frame (permuto_sdf_py/utils/common_utils.py:573-589) for the camera-frame normals, for the chunk
   [pixel_first, pixel_first + nr_rays) of an H x W frame.  slot [nr_rays] from psdf_trace_frame_select; origins, dirs
   [nr_rays, 3] the chunk's rays; pos, gradients, rgb [nr_valid, 3] the end points, SDF gradients and colours of the valid rays
   (may be NULL with nr_valid = 0); rot_cam_world: device pointer to the 9 floats of the row-major rotation of tf_cam_world, read
   when normals_cam_img is given.  Written at pixel pixel_first + ray, for a valid ray / any other: rgb_img [3, H, W] <- its rgb
   row / 0; normals_img [3, H, W] <- g / max(|g|, 1e-12) / 0; normals_cam_img [3, H, W] or NULL <- normalize(R n) / 0;
   weights_sum_img [1, H, W] <- 1 / 0; depth_img [1, H, W] <- ((px - ox) dx + (py - oy) dy) + (pz - oz) dz / 0 (not in the
   reference).  One weight-1 sample per ray: colours and gradients are copied, not summed.  nr_rays = 0 returns 0 without a
   launch; -1 for nr_rays < 0, nr_valid outside [0, nr_rays], a NULL pointer, an extent < 1 or a range outside the frame; -2 for
   H W >= 2^31. */
int psdf_trace_frame_resolve(int nr_rays, int nr_valid, const int* slot, const float* origins, const float* dirs, const float*
    pos, const float* gradients, const float* rgb, const float* rot_cam_world, int H, int W, int64_t pixel_first, float* rgb_img,
    float* normals_img, float* normals_cam_img, float* weights_sum_img, float* depth_img, void* stream);

/* ---- box_trace.hip ---- */
/* Sphere tracing inside an axis-aligned box without an occupancy grid, one slot per ray, and the image planes of such a view.
   The box comes as HOST triples computed by the caller in float32 in the reference's order (permuto_sdf_py/utils/aabb.py:15-25,
   48-49): box_min = -sizes / 2 + translation, box_max = sizes - sizes / 2 + translation (the intersection); translation and
   half = sizes / 2 (the inside test).  origins, dirs [nr_rays, 3]; points are rows of `stride` floats, stride 3, or 4 with the
   time in column 3; flags are bytes.  The entries allocate nothing and never synchronise; nr_rays = 0 returns 0 without a
   launch; -1 for nr_rays < 0, a stride other than 3 or 4, or a NULL required pointer. */
/* replaces: AABB.ray_intersection (permuto_sdf_py/utils/aabb.py:47-100), operation for operation: IEEE division per axis (a
   direction component of +-0 included), the swap, lo / hi from -+1e10, the two miss conditions, both depths 0 on a miss, lo
   clamped at 0, origin + t * dir as a product and a sum -> t_entry, t_exit [nr_rays], pts_entry, pts_exit [nr_rays, 3], hit
   [nr_rays] */
int psdf_box_ray_intersection(int nr_rays, const float* box_min, const float* box_max, const float* origins, const float* dirs,
    float* t_entry, float* t_exit, float* pts_entry, float* pts_exit, uint8_t* hit, void* stream);
/* replaces: the start of sphere_trace without an occupancy grid (permuto_sdf_py/utils/sdf_utils.py:122, 136-144): pts [nr_rays,
   stride] <- the entry point (the origin for a ray that misses the box), column 3 <- time[0] with stride 4 (time: DEVICE pointer
   to one float, read by the kernel: a captured launch follows it; may be NULL with stride 3); converged = no_hit <- !hit (a ray
   that misses is held as converged and never evaluated; the reference traces it from the camera centre) */
int psdf_box_trace_begin(int nr_rays, int stride, const float* box_min, const float* box_max, const float* origins, const float*
    dirs, const float* time, float* pts, uint8_t* converged, uint8_t* no_hit, void* stream);
/* replaces: one iteration of that loop after the network (sdf_utils.py:167-185) with check_point_inside_primitive
   (aabb.py:28-42), for the rays with converged == 0: p <- p + (d * sdf) * multiplier; converged |= |sdf| < thresh (the SDF from
   before the move) || !(p - translation strictly between -half and half on all three axes).  Column 3 is never touched; rays
   with converged != 0 are not touched at all */
int psdf_box_trace_step(int nr_rays, int stride, const float* translation, const float* half, const float* dirs, const float* sdf,
    float multiplier, float thresh, float* pts, uint8_t* converged, void* stream);
/* replaces: filter_unconverged_points (sdf_utils.py:221-231), F.normalize and the convergence mask of
   permuto_sdf_py/experiments/visualization/vis_4d_sdf.py:106-118, as planes, for the chunk [pixel_first, pixel_first + nr_rays)
   of an H x W frame.  A ray is covered iff !no_hit && sdf_end < coverage_thresh (a signed compare; a NaN is not covered).
   Written at pixel pixel_first + ray, for a covered ray / any other: normals_img [3, H, W] <- g / max(|g|, 1e-12), g =
   gradients[ray, 0:3] (rows of `stride` floats, as pts) / 0; normals_cam_img [3, H, W] or NULL <- normalize(R n), R =
   rot_cam_world (device, 9 floats, row major) / 0; weights_sum_img [1, H, W] <- 1 / 0; depth_img [1, H, W] <- ((px - ox) dx +
   (py - oy) dy) + (pz - oz) dz / 0.  Every pixel of the range is written once, nothing outside it.  Also -1 for an extent < 1,
   a range outside the frame or camera normals without the rotation; -2 for H W >= 2^31 */
int psdf_box_trace_resolve(int nr_rays, int stride, const float* origins, const float* dirs, const float* pts, const float*
    sdf_end, const float* gradients, const uint8_t* no_hit, float coverage_thresh, const float* rot_cam_world, int H, int W,
    int64_t pixel_first, float* normals_img, float* normals_cam_img, float* weights_sum_img, float* depth_img, void* stream);

/* ---- sdf_slice.hip ---- */
/* Cross-sections of an SDF: the layer of points of create_sdf_isolines, its colour map with iso-bands, and the depth test of
   the layer against a rendered view.  The plane comes as HOST values: axes, 9 floats of a row-major 3 x 3 matrix whose COLUMNS
   are the plane's axes (the reference's cam.cam_axes()), the layer depth z along the third axis and the half width of the
   layer (extent_scale; 1 is the reference's [-1, 1)).  The box comes as the host triples translation and half = sizes / 2 of
   psdf_box_trace_step.  Points are rows of `stride` floats, stride 3, or 4 with the time in column 3 (time: DEVICE pointer to
   one float, may be NULL with stride 3); flags are bytes.  The colour arguments are: table [K, 3] on the DEVICE, 2 <= K <=
   65536; base_map, 4 HOST floats (in_lo, in_hi, out_lo, scale) of a map_range whose scale = (out_hi - out_lo) / (in_hi - in_lo)
   the caller computed in float64 and rounded; nr_lines <= 32 bands as the HOST arrays band_lo, band_hi [nr_lines] and band_rgb
   [nr_lines, 3] (may be NULL with nr_lines = 0).  The colour of a value s is 0 for a NaN, else table(base_map(s)) -- overwritten
   by band_rgb[i] of the LAST i with s > band_lo[i] && s < band_hi[i] (float32, both strict).  csrc/sdf_slice.hip states the
   evaluation order of table() and of the rotation, both restated and unpinned.  The entries allocate nothing and never
   synchronise; a count of 0 returns 0 without a launch; -1 for a negative count, a stride other than 3 or 4, nr_lines outside
   [0, 32], K outside [2, 65536], an extent < 1, a range outside the layer or the frame, or a NULL required pointer; -2 for
   S S >= 2^31 or H W >= 2^31. */
/* replaces: the layer of create_sdf_isolines (permuto_sdf_py/experiments/visualization/visualize_sdf_isolines.py:69-92, 96-101;
   render_from_frame.py:71-166 and sample_sdf_in_layer of permuto_sdf_py/utils/sdf_utils.py build the same layer) and
   AABB.check_point_inside_primitive (permuto_sdf_py/utils/aabb.py:28-42) on it, for the cells [first, first + count) of an
   S x S layer; cell k has row k / S (y) and column k % S (x).  pts [count, stride] <- the rotated cell (float32 lattice, float64
   rotation rounded once), column 3 <- time[0] with stride 4; skip [count] <- !(strictly inside the box) */
int psdf_slice_points(int S, int64_t first, int count, int stride, const float* axes, float z, float extent_scale, const float*
    translation, const float* half, const float* time, float* pts, uint8_t* skip, void* stream);
/* replaces: the colour map and the 15 masked assignments of visualize_sdf_isolines.py:111-138 (map_range_tensor,
   permuto_sdf_py/utils/common_utils.py:150-154; the defaults of src/NGPGui.cxx:22-25) and remove_marked_vertices (:153-156), for
   the same cells: sdf, skip [count] -> at cell first + i of the planes rgb [3, S, S] <- the colour, sdf_img [1, S, S] <- sdf,
   inside_img [1, S, S] <- 1; a skipped cell gets 0 in all three.  Every cell of the range is written once, nothing outside it */
int psdf_slice_colorize(int S, int64_t first, int count, const float* sdf, const uint8_t* skip, const float* table, int K, const
    float* base_map, int nr_lines, const float* band_lo, const float* band_hi, const float* band_rgb, float* rgb, float*
    sdf_img, float* inside_img, void* stream);
/* replaces: the viewer's depth test of the layer against the scene (Scene.show, visualize_sdf_isolines.py:158-162, and
   render_easypbr_from_frame :171-203), first half, for the rays [pixel_first, pixel_first + nr_rays) of an H x W frame (origins,
   dirs [nr_rays, 3] as from psdf_frame_rays).  With n the third axis: t = dot(n, z n - o) / dot(n, d), p = o + t d, all float32.
   A ray takes part iff dot(n, d) != 0, t > 0, dot(a0, p) and dot(a1, p) lie in [-extent, extent), p is strictly inside the
   box, and weights_sum_img[pixel] == 0 || t < depth_img[pixel].  pts [nr_rays, stride] <- p (the origin for a ray that does
   not take part), column 3 <- time[0]; skip [nr_rays] <- !takes part; t [nr_rays] <- t (0 for a ray that does not) */
int psdf_slice_cut_begin(int nr_rays, int stride, const float* axes, float z, float extent, const float* translation, const
    float* half, const float* origins, const float* dirs, const float* time, int H, int W, int64_t pixel_first, const float*
    weights_sum_img, const float* depth_img, float* pts, uint8_t* skip, float* t, void* stream);
/* replaces: the second half of the same (visualize_sdf_isolines.py:158-162 with the colours of :111-138), after the network:
   for a ray with skip == 0, rgb_img [3, H, W] <- the colour of sdf[ray], depth_img <- t[ray], weights_sum_img <- 1,
   slice_mask_img [1, H, W] <- 1, in place at pixel pixel_first + ray; for any other ray slice_mask_img <- 0 and the other planes
   keep their bits */
int psdf_slice_cut_resolve(int nr_rays, const float* sdf, const uint8_t* skip, const float* t, const float* table, int K, const
    float* base_map, int nr_lines, const float* band_lo, const float* band_hi, const float* band_rgb, int H, int W, int64_t
    pixel_first, float* rgb_img, float* depth_img, float* weights_sum_img, float* slice_mask_img, void* stream);

/* ---- colorcal.hip ---- */
/* Per-image colour calibration of NeRF training (permuto_sdf_py/train_nerf.py:52,158-161; Colorcal, models.py:678-729), applied
   to the raw colours of a packed container before the sigmoid (models.py:520-523).  Ray-index arguments as
   psdf_nerf_render_forward (the compacted form and the equal-count form with implicit ranges); nr_samples M; img_idx [R] int32
   the image of every ray; weight_delta, bias [nr_images, 3].  A ray of image idx_fixed, and a ray whose img_idx lies outside
   [0, nr_images), keeps the identity (w = 1, b = 0) and the tables are not read for it.  A ray is processed when RayIndex
   accepts it and its range lies inside [0, M].  The entries allocate nothing and never synchronise; nr_rays <= 0 returns 0
   before any pointer is looked at (nothing is written).  -1: nr_samples < 0, nr_images < 1, idx_fixed outside [0, nr_images), a
   NULL pointer that is needed; -2: nr_rays > 2^31 - 1 - 2^18, nr_samples > (2^31 - 1) / 3, nr_images > 2^24. */
/* replaces: Colorcal.calib_RGB_samples_packed (models.py:693-729) + the sigmoid (models.py:520-523) on the colour head's
   feature-major output raw_fm [3, M] -> rgb [M, 3] = 1 / (1 + expf(-z)), z = raw * (1 + weight_delta[img]) rounded, + bias[img]
   rounded.  With w = 1, b = 0 the bits of psdf_sigmoid_rows.  Slots no processed ray owns are not written.  nr_samples == 0
   returns 0 as well. */
int psdf_colorcal_sigmoid_forward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int64_t nr_samples,
    const float* raw_fm, const int* img_idx, int nr_images, int idx_fixed, const float* weight_delta, const float* bias, float*
    rgb, void* stream);
/* Backward of the above for grad_rgb [M, 3], with rgb [M, 3] (the forward's output) and raw_fm [3, M]: grad_raw_fm [3, M] <-
   g_pre w, g_pre = grad_rgb rgb (1 - rgb) (slots no processed ray owns are not written); grad_ray [R, 6] <- per ray the sums
   over its samples of g_pre raw (columns 0-2) and of g_pre (columns 3-5).  Every row of grad_ray is written: zeros for rays that
   are not processed and for rays that keep the identity.  The order of a ray's sums depends on its sample count alone (16
   lanes take the samples in turn, then a fixed butterfly): no atomics, the same inputs give the same bits on every call.  With
   nr_samples == 0 the sample pointers and the tables may be NULL. */
int psdf_colorcal_sigmoid_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int64_t nr_samples,
    const float* grad_rgb, const float* rgb, const float* raw_fm, const int* img_idx, int nr_images, int idx_fixed, const float*
    weight_delta, const float* bias, float* grad_raw_fm, float* grad_ray, void* stream);
/* replaces: the two index_add_ of torch autograd through Colorcal's index_select.  grad_ray_a [R, 6], grad_ray_b [R, 6] or NULL
   (a second branch: the background's) -> grad_weight_delta [nr_images, 3] <- for every image the sum over its rays, in
   ascending ray order, of (grad_ray_b[r] + grad_ray_a[r]) columns 0-2, grad_bias [nr_images, 3] <- of columns 3-5.  Every entry
   is written; the row of idx_fixed and of an image no ray drew is exactly 0.  Deterministic. */
int psdf_colorcal_fold(int nr_rays, const int* img_idx, int nr_images, int idx_fixed, const float* grad_ray_a, const float*
    grad_ray_b, float* grad_weight_delta, float* grad_bias, void* stream);

/* ---- frame_composite.hip: views of a NeRF ---- */
/* replaces: train_nerf.py:66-71,92-128 -- per chunk, NerfHash's softplus, VolumeRenderingNerf.compute_weights + integrate of
   the FOREGROUND as run_net calls them, and the list appends, torch.cat and lin2nchw of run_net_in_chunks around it.  Ray-index
   and sample arguments as psdf_nerf_render_forward; z [M] the samples' depth along their ray; H, W, pixel_first as in the
   section below.  Written at pixel pixel_first + ray: rgb_img [3, H, W] <- sum w rgb; weights_sum_img [1, H, W] <- sum w;
   depth_img [1, H, W] or NULL <- sum w z, summed as a colour channel is (not in the reference; with NULL z is not read and may
   be NULL); transmittance [nr_rays] <- T of the ray's last sample, what psdf_frame_composite_nerf of the same chunk reads.
   The sweep and the order of summation are psdf_nerf_render_forward's: the planes hold its bits.  Empty and overflowed rays: 0,
   0, 0 and 1.  Any ray length.  With max_nr_samples = 0 the sample pointers may be NULL.  Allocates nothing and never
   synchronises; nr_rays <= 0 returns 0 before any pointer check; -1 for a NULL required pointer (z with depth_img and
   max_nr_samples > 0 among them), max_nr_samples < 0, equal with fixed < 0, an extent < 1 or a range outside the frame; -2 for
   H W >= 2^31 */
int psdf_nerf_frame_render(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float*
    raw_density, const float* dt, const float* z, const float* rgb, int H, int W, int64_t pixel_first, float* rgb_img, float*
    weights_sum_img, float* depth_img, float* transmittance, void* stream);

/* ---- frame_rays.hip, frame_composite.hip ---- */
/* A held-out view rendered volumetrically, a chunk of pixels at a time, into planar [3, H, W] / [1, H, W] fp32 images on the
   device.  Pixel p of an H x W frame is (x, y) = (p % W, p / W) with its centre at +0.5; a chunk is the pixel range
   [pixel_first, pixel_first + nr_rays) and ray r of a chunk's sample container belongs to pixel pixel_first + r.  The entries
   allocate nothing and never synchronise; nr_rays <= 0 returns 0 before any pointer check; -1 for a NULL pointer, an extent < 1
   or a range outside the frame, -2 for H W >= 2^31. */
/* host only: the chunking of a frame (csrc/frame_plan.h) -> out [PSDF_FRAME_PLAN_FIELDS] int64: 0 rays per chunk, the largest
   multiple of 64 with rays * max_nr_samples_per_ray <= pool_samples (the condition under which no ray of a chunk overflows the
   march's sample pool), at most H W; 1 the number of chunks; 2 the rays of the last chunk.
   replaces: the fixed chunk_size = 3000 of permuto_sdf_py/experiments/evaluation/create_my_images.py:80 and the chunk
   arithmetic of run_net_in_chunks (permuto_sdf_py/train_permuto_sdf.py:174-176).
   -1: H, W or max_nr_samples_per_ray < 1, pool_samples < 64 * max_nr_samples_per_ray, out NULL; -2: H W >= 2^31 */
#define PSDF_FRAME_PLAN_FIELDS 3
int psdf_frame_plan(int H, int W, int max_nr_samples_per_ray, int64_t pool_samples, int64_t* out);
/* replaces: create_rays_from_frame (permuto_sdf_py/utils/nerf_utils.py:459-500) for a range of pixels.  K: device pointer to
   the 9 floats of one row-major intrinsic matrix, tf_world_cam: to the 16 floats of one row-major [R|t] (what a reel holds per
   image); origins [nr_rays, 3], dirs [nr_rays, 3].  The arithmetic is psdf_random_rays_from_reel's: the ray of a pixel has the
   same bits from both. */
int psdf_frame_rays(int H, int W, const float* K, const float* tf_world_cam, int64_t pixel_first, int nr_rays, float* origins,
    float* dirs, void* stream);
/* replaces: per chunk, compute_weights + integrate of the colours and of the SDF gradients + F.normalize of run_net
   (permuto_sdf_py/train_permuto_sdf.py:137-142), the list appends, torch.cat and lin2nchw of run_net_in_chunks (:190-207), and
   rotate_normals_to_cam_frame (permuto_sdf_py/utils/common_utils.py:573-589).  Ray-index and sample arguments as
   psdf_neus_composite_forward; rot_cam_world: device pointer to the 9 floats of the row-major rotation of tf_cam_world, read
   when normals_cam_img is given.  Written at pixel pixel_first + ray: rgb_img [3, H, W] <- sum w rgb; normals_img [3, H, W] <-
   G / max(|G|, 1e-12), G = sum w gradient; normals_cam_img [3, H, W] or NULL <- normalize(R n); weights_sum_img [1, H, W] <-
   sum w; transmittance [nr_rays] <- the background transmittance of every ray of the chunk.  Empty and overflowed rays: 0, 0,
   0, 0 and 1 (:124-129).  Any ray length.  With max_nr_samples = 0 the sample pointers may be NULL. */
int psdf_frame_composite_neus(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* sdf,
    const float* dirs, const float* gradients, const float* dt, const float* rgb, const float* inv_s, float cos_anneal_ratio,
    const float* rot_cam_world, int H, int W, int64_t pixel_first, float* rgb_img, float* normals_img, float* normals_cam_img,
    float* weights_sum_img, float* transmittance, void* stream);
/* replaces: the background half of run_net (permuto_sdf_py/train_permuto_sdf.py:156-162) and its share of the cat / lin2nchw
   of run_net_in_chunks.  Arguments as psdf_nerf_composite_forward; transmittance [nr_rays] and the foreground already in
   rgb_img come from psdf_frame_composite_neus of the same chunk.  rgb_bg_img [3, H, W] <- t * (sum w rgb); rgb_img <- rgb_img +
   that.  Rays without background samples add 0. */
int psdf_frame_composite_nerf(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float*
    raw_density, const float* dt, const float* rgb, const float* transmittance, int H, int W, int64_t pixel_first, float*
    rgb_img, float* rgb_bg_img, void* stream);

/* ---- mesh_color.hip ---- */
/* Per-vertex colour of an extracted surface: the glue around the colour network (RgbNet, models.py:310-391) when it is asked
   about the n vertices of a mesh.  x_fm [C, n] is the network's feature-major input, rows [colour encoding | 25 SH values of
   degree 5 of the view direction | unit normal | g geometry features]; the colour encoding's rows are written by
   psdf_encode_forward into the same buffer.  The entries allocate nothing and never synchronise; n == 0 returns 0 before any
   pointer is looked at; -1: n < 0 or an argument below; -2: n > 2^31 - 1 vertices in one launch, C > 2^16. */
/* host only: the rows of x_fm and the chunks of a call (csrc/mesh_color_plan.h) -> out [PSDF_MESH_COLOR_PLAN_FIELDS] int64: 0
   c_enc, the row at which the SH block starts (= rgb_enc_width); 1 c_sh, at which the normal starts; 2 c_normal, at which the
   geometry features start; 3 c_geom, one past them; 4 C = c_geom; 5 the number of chunks of n vertices in chunks of `chunk`; 6 the
   vertices of the last chunk (0, 0 for n == 0).  -1: rgb_enc_width < 1, g < 0, C != mlp_in (the width the colour MLP takes),
   n < 0, chunk < 1, out NULL; -2: C > 2^16, chunk > 2^31 - 1 */
#define PSDF_MESH_COLOR_PLAN_FIELDS 7
int psdf_mesh_color_plan(int rgb_enc_width, int g, int mlp_in, int64_t n, int64_t chunk, int64_t* out);
/* replaces, for vertices: PermutoSDF.spherical_harmonics + F.normalize + the torch.cat (with its transposes) of RgbNet.forward
   (models.py:352-372).  points [n, 3]; gradients [n, 3] the SDF gradients; y_fm [1 + g, n] the SDF net's feature-major output
   (row 0, the SDF, is not read).  Per vertex: nrm = G / max(|G|, 1e-12) (the bits of psdf_normalize3); view direction d = -nrm
   (mode 0: the surface seen head-on from outside) or (p - eye) / max(|p - eye|, 1e-12) (mode 1; eye: device pointer to 3
   floats; points is read in this mode only); rows [sh_row, sh_row + 25) of x_fm <- the SH values of d (the bits of
   psdf_spherical_harmonics), rows [sh_row + 25, sh_row + 28) <- nrm, rows [sh_row + 28, sh_row + 28 + g) <- rows 1 .. g of
   y_fm; dirs [n, 3] or NULL <- d; normals [n, 3] or NULL <- nrm.  Rows [0, sh_row) are not touched.  A zero gradient gives
   nrm = 0 and d = 0 (no special case).  -1: g < 0, sh_row < 0, a mode other than 0 and 1, sh_row + 28 + g != C, a NULL pointer
   that is read or x_fm NULL. */
int psdf_mesh_color_inputs(int64_t n, const float* points, const float* gradients, const float* y_fm, int g, int mode, const
    float* eye, float* x_fm, int C, int sh_row, float* dirs, float* normals, void* stream);
/* replaces, for vertices: torch.sigmoid of RgbNet.forward (models.py:391) and the 8-bit conversion of the views (image_eval.to_u8) on the
   colour head's feature-major output raw_fm [3, n] -> rgb [n, 3] or NULL <- 1 / (1 + expf(-raw)) (the bits of
   psdf_sigmoid_rows); rgb_u8 [n, 3] uint8 or NULL <- clamp(rint(rgb * 255), 0, 255), ties to even.  -1: raw_fm NULL. */
int psdf_mesh_color_finish(int64_t n, const float* raw_fm, float* rgb, uint8_t* rgb_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSDF_H */
