/*
 * hgs_rast.h - C ABI of libhgs_rast.so, the MI355X (gfx950) differentiable 3D Gaussian
 * Splatting rasterizer that drops in behind HumanGaussian's
 * `diff_gaussian_rasterization` extension.
 *
 * The reference has no C ABI: its boundary is the pybind11 module
 * `diff_gaussian_rasterization._C` of the un-vendored ashawkey fork, reached from
 *   /root/reference/gaussiansplatting/gaussian_renderer/__init__.py:14,36-51,86-94
 *   /root/reference/gs_renderer.py:10-13,951-966,1006-1015
 * Each entry point below names the `_C` function it replaces.  Conventions:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says HOST;
 *   - the caller owns every buffer; the library never allocates, frees or synchronises;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no global state,
 *     so calls on distinct streams / devices may run concurrently;
 *   - return value: 0 on success, a negative HGS_E* code for argument errors, or
 *     -(1000 + hipError_t) when a launch fails.  Nothing throws across the ABI.
 *   - tensors are fp32, contiguous, row-major with the shapes of SURVEY.md section 3.3.
 */
#ifndef HGS_RAST_H
#define HGS_RAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGS_MAX_VIEWS 16  /* views (cameras) one batched call can take */
#define HGS_MAX_ENTRY_CAPACITY (1ll << 27)  /* entry ids travel in 27 bits: hgs_forward* / hgs_backward* return HGS_EINVAL for a larger
                                               entry_capacity (134 M tile-list entries = ~45 GB of bin buffer per call) */

#define HGS_OK 0
#define HGS_EINVAL (-1)   /* bad argument (null pointer, negative size, ...) */
#define HGS_ESHAPE (-2)   /* "exactly one of shs / colors_precomp", "scales+rotations / cov3D" */

/* Mirrors GaussianRasterizationSettings, same field order as the reference call site
 * gaussian_renderer/__init__.py:36-49.  bg / viewmatrix / projmatrix / campos stay on the
 * device (the reference hands over CUDA tensors); matrices are the row-major bytes of the
 * (4,4) tensors, i.e. viewmatrix = w2c^T, projmatrix = viewmatrix @ P^T (cameras.py:50-52). */
typedef struct hgs_settings {
  int32_t image_height;
  int32_t image_width;
  float tanfovx;
  float tanfovy;
  const float* bg;          /* [3]  */
  float scale_modifier;
  const float* viewmatrix;  /* [16] */
  const float* projmatrix;  /* [16] */
  int32_t sh_degree;        /* ACTIVE degree (0..3) */
  const float* campos;      /* [3]  */
  int32_t prefiltered;
  int32_t debug;
} hgs_settings;

/* Written by hgs_forward into the tail of the geom buffer (device) and, once the stream
 * reaches that point, mirrored to `status_host` (HOST, pinned) when it is non-NULL. */
typedef struct hgs_status {
  uint32_t num_rendered;   /* R = entries in the tile lists.  <= upstream's `num_rendered`: a    */
                           /* (Gaussian, tile) pair gets an entry only if the box of its         */
                           /* alpha >= 1/255 ellipse touches the tile (results are unchanged)    */
  uint32_t active_tiles;   /* tiles with a non-empty list                              */
  uint32_t num_pairs;      /* (entry, 4x4-pixel cell) pairs = the pair rows of the backward scratch.  Known */
                           /* only when the sort has run: 0 in what the status mirror / event delivers, set */
                           /* in the device copy and in a MAPPED host mirror when the blend forward starts  */
                           /* (a host that finds it non-zero later may size the scratch by it, see          */
                           /* hgs_bwd_scratch_bytes_pairs; 0 = not known (yet): size for the worst case).   */
                           /* LIFETIME: a mapped mirror is therefore written a SECOND time, after the ready */
                           /* word reserved[2]: it must stay valid (not freed, not reused for another call) */
                           /* until the forward's stream work has completed, not merely until the poll ends */
  uint32_t bwd_groups;     /* unused since ABI v11 (0): the blend kernels run persistent waves */
  uint32_t overflow;       /* != 0: outputs are INVALID.  bit0: R exceeded              */
                           /* entry_capacity (retry with >= num_rendered); bit1: a tile */
                           /* list exceeded max_tile_entries_hint (retry with hint 0)   */
  uint32_t reserved[3];    /* [0] = entry_capacity the bin buffer was carved with,      */
                           /* [1] = longest tile list, [2] = 1: "complete" - in the host mirror this */
                           /* word is stored LAST behind a system-scope fence, so a host that  */
                           /* cleared it before the call may POLL it instead of using an event */
} hgs_status;

/* ---- buffer sizing (host-side arithmetic, no device work) --------------------------
 * Replaces the three resize callbacks (geometry / binning / image state) that upstream's
 * rasterize_gaussians() drives through torch.  geom: per-Gaussian + per-tile state;
 * bin: per-(tile,Gaussian) entry state, sized by entry_capacity; img: per-pixel state;
 * bwd_scratch: gradient rows per entry and per (entry, 4x4-pixel cell) pair, used only inside
 * hgs_backward (48 + 16 x 40 B per entry). */
size_t hgs_geom_bytes(int32_t P, int32_t image_height, int32_t image_width);
size_t hgs_bin_bytes(int64_t entry_capacity);
size_t hgs_img_bytes(int32_t image_height, int32_t image_width);
size_t hgs_bwd_scratch_bytes(int64_t num_rendered);
/* the same with the pair rows counted instead of bounded (hgs_status.num_pairs of THAT forward call, once
 * published; ~4.4 per entry on an avatar instead of 16): 48 B per entry + 40 B per pair */
size_t hgs_bwd_scratch_bytes_pairs(int64_t num_rendered, int64_t num_pairs);
/* the same for a batch of B views (geom / img scale with B; the bin buffer and the backward
 * scratch are sized by the entry capacity / num_rendered of ALL views together) */
size_t hgs_geom_bytes_batch(int32_t B, int32_t P, int32_t image_height, int32_t image_width);
size_t hgs_img_bytes_batch(int32_t B, int32_t image_height, int32_t image_width);

/* Optional per-stage timing (measurement only; pass NULL in production): `stage_events`
 * is a HOST array of hipEvent_t handles; entry k (if non-NULL) is recorded on `stream`
 * after stage k.  Forward: 0 start, 1 preprocess, 2 tile tables, 3 fill (+ status), 4 sort, 5 blend.
 * Backward: 0 start, 1 blend backward, 2 pair reduction, 3 preprocess backward. */
#define HGS_FWD_STAGES 6
#define HGS_BWD_STAGES 4

/* ---- forward: replaces _C.rasterize_gaussians --------------------------------------
 * Exactly one of shs / colors_precomp and exactly one of {scales,rotations} /
 * cov3D_precomp must be non-NULL (HGS_ESHAPE otherwise), matching the fork's Python
 * checks.  shs is (P, M, 3); M = max coefficient count of the tensor.
 * out_color (3,H,W), out_depth (1,H,W), out_alpha (1,H,W), radii (P) int32.
 * store_bwd_state = 0 skips the pixel-state stores the backward needs (no-grad / inference calls).
 * max_tile_entries_hint: 0 = unknown; > 0 = the caller promises no tile list is longer
 * (lets the library skip launching sort classes that cannot occur); a broken promise is
 * detected on the device and reported as overflow bit 1 (value 2) - call again with 0.
 * P == 0 writes background / zeros and reports num_rendered = 0.
 * status_host_mapped != 0: `status_host` is pinned host memory that the device can address
 * with the same pointer (hipHostMalloc / torch pin_memory on ROCm); the fill launch then
 * stores the status into it directly (system-scope fence) and no copy is enqueued.
 * Otherwise the status copy to `status_host` is enqueued right after the fill stage (before
 * sort / blend); `status_event` (a hipEvent_t, may be NULL) is recorded right behind it, so a
 * host can wait for just the status - hipEventSynchronize(status_event) - while the rest of
 * the forward is still running, and knows about an overflow before it hands out outputs. */
int hgs_forward(const hgs_settings* s, int32_t P, int32_t M,
                const float* means3D, const float* shs, const float* colors_precomp,
                const float* opacities, const float* scales, const float* rotations,
                const float* cov3D_precomp,
                float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                void* geom, void* bin, int64_t entry_capacity, void* img,
                int32_t store_bwd_state, int32_t max_tile_entries_hint,
                hgs_status* status_host, int32_t status_host_mapped, void* status_event,
                void* const* stage_events, void* stream);

/* ---- batched forward: B views of the same Gaussians in ONE launch set ----------------
 * Replaces the per-view Python loop around _C.rasterize_gaussians at
 * /root/reference/threestudio/systems/GaussianDreamer.py:244-266 (8 views per training step).
 * `views` is a HOST array of B settings (1 <= B <= HGS_MAX_VIEWS) that must agree in
 * image_height / image_width / sh_degree / scale_modifier and may differ in everything a camera
 * carries (tanfov, matrices, campos, bg).  Outputs are [B][3][H][W], [B][1][H][W], [B][1][H][W]
 * and radii [B][P]; each view's result is bit-identical to a separate hgs_forward call.  One
 * status for the whole batch (num_rendered = sum over views).  hgs_forward IS this function
 * with B = 1; buffers are sized with the *_batch sizing functions. */
int hgs_forward_batch(const hgs_settings* views, int32_t B, int32_t P, int32_t M,
                      const float* means3D, const float* shs, const float* colors_precomp,
                      const float* opacities, const float* scales, const float* rotations,
                      const float* cov3D_precomp,
                      float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                      void* geom, void* bin, int64_t entry_capacity, void* img,
                      int32_t store_bwd_state, int32_t max_tile_entries_hint,
                      hgs_status* status_host, int32_t status_host_mapped, void* status_event,
                      void* const* stage_events, void* stream);

/* ---- batched backward ----------------------------------------------------------------
 * dL_dout_* are [B][..] like the outputs.  Parameter gradients are the SUM over the views, formed
 * in view order 0..B-1 inside one kernel (deterministic; what autograd accumulates over the
 * reference's loop); dL_dmeans2D stays per view, [B][P][3], because the caller consumes it per
 * view (GaussianDreamer.py:385-387).  radii is [B][P]. */
int hgs_backward_batch(const hgs_settings* views, int32_t B, int32_t P, int32_t M,
                       const float* means3D, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, const float* rotations,
                       const float* cov3D_precomp, const int32_t* radii,
                       const float* out_color, const float* out_depth, const float* out_alpha,
                       const float* dL_dout_color, const float* dL_dout_depth,
                       const float* dL_dout_alpha,
                       const void* geom, const void* bin, const void* img,
                       const hgs_status* status, int64_t entry_capacity, void* bwd_scratch,
                       float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                       float* dL_dcolors_precomp, float* dL_dopacities, float* dL_dscales,
                       float* dL_drotations, float* dL_dcov3D_precomp,
                       void* const* stage_events, void* stream);

/* ---- fused activations -----------------------------------------------------
 * The reference feeds the rasterizer `get_opacity` = sigmoid(_opacity), `get_scaling` = exp(_scaling),
 * `get_rotation` = normalize(_rotation) (gaussiansplatting/scene/gaussian_model.py:95-115): three
 * elementwise kernels forward and three backward per render call.  With the *_act entry points the
 * caller hands over the RAW parameters and the activation runs inside the per-Gaussian kernels
 * (forward: as the value is loaded; backward: chain rule applied to the summed gradient, so
 * dL_dopacities / dL_dscales / dL_drotations are gradients w.r.t. the raw parameters).
 * activation_flags: any combination of the HGS_ACT_* bits below (+ HGS_GRAD_SCALE_TRUE_DERIVATIVE for the backward);
 * 0 = identical to the plain entry points. */
#define HGS_ACT_OPACITY_SIGMOID 1    /* opacities are logits                                  */
#define HGS_ACT_SCALE_EXP 2          /* scales are log-scales                                 */
#define HGS_ACT_ROTATION_NORMALIZE 4 /* rotations are un-normalised quaternions (w,x,y,z)      */
/* Backward only (ignored by the forward).  dL_dscales at scale_modifier != 1: the fork's backward (computeCov3D:
 * `s = mod * scale`, `dL_dscale = dot(Rt[i], dL_dMt[i])`) returns dL/d(mod * scale) - the modifier's factor is missing -
 * and that is what this library returns by default, like the extension it replaces (identical at 1.0, the only value
 * the reference passes: gaussian_renderer/__init__.py:18, gs_renderer.py:925).  With this bit set dL_dscales is the
 * true derivative dL/dscale = mod * dL/d(mod * scale). */
#define HGS_GRAD_SCALE_TRUE_DERIVATIVE 8
/* v17, opt-in antialiasing: the screen-space filter of Mip-Splatting (upstream 3DGS's `antialiasing` switch).  Every
 * projected covariance gets the 0.3 px^2 dilation as always; with this bit each Gaussian's opacity is also scaled by
 *   rho = sqrt(max(2.5e-5, det(Sigma2D) / det(Sigma2D + 0.3 I)))
 * so that the dilation adds no coverage (radii, tile rects and tiles_touched stay exactly as without the bit: the rects are
 * cut with the opacity before the factor).  dL_dopacities is then
 * the gradient w.r.t. the opacity before the factor, and the backward carries rho's dependence on the covariance into
 * the mean, scale, rotation and cov3D gradients.  Accepted by hgs_forward_batch_act(_leaf), hgs_backward_batch_act and
 * hgs_backward_batch_packed.  Like entry_capacity, the bit must be the SAME in the forward and the backward of a call
 * (the backward recomputes rho; it does not check the forward's choice); the backward with it needs `opacities`. */
#define HGS_ANTIALIAS 16
int hgs_forward_batch_act(const hgs_settings* views, int32_t B, int32_t P, int32_t M,
                          const float* means3D, const float* shs, const float* colors_precomp,
                          const float* opacities, const float* scales, const float* rotations,
                          const float* cov3D_precomp,
                          float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                          void* geom, void* bin, int64_t entry_capacity, void* img,
                          int32_t store_bwd_state, int32_t max_tile_entries_hint,
                          hgs_status* status_host, int32_t status_host_mapped, void* status_event,
                          void* const* stage_events, int32_t activation_flags, void* stream);
/* v16: hgs_forward_batch_act that also ZERO-FILLS the caller's screen-space leaf.  The reference creates
 * `screenspace_points = torch.zeros_like(xyz) + 0` per view (gaussian_renderer/__init__.py:26) only to receive
 * dL/dmeans2D in its .grad: a fill (and an add) launch in front of every forward.  means2D_leaf [B][P][3] (or NULL:
 * exactly hgs_forward_batch_act) is written with zeros by the per-Gaussian kernel of the forward itself - row (b, i) by
 * the thread that projects Gaussian i of view b - so the caller hands over UNINITIALISED storage and reads zeros behind
 * the call: no launch, no kernel boundary (2.6 us of a 158 us step at 100k Gaussians). */
int hgs_forward_batch_act_leaf(const hgs_settings* views, int32_t B, int32_t P, int32_t M,
                               const float* means3D, const float* shs, const float* colors_precomp,
                               const float* opacities, const float* scales, const float* rotations,
                               const float* cov3D_precomp,
                               float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                               void* geom, void* bin, int64_t entry_capacity, void* img,
                               int32_t store_bwd_state, int32_t max_tile_entries_hint,
                               hgs_status* status_host, int32_t status_host_mapped, void* status_event,
                               void* const* stage_events, int32_t activation_flags, float* means2D_leaf, void* stream);
int hgs_backward_batch_act(const hgs_settings* views, int32_t B, int32_t P, int32_t M,
                           const float* means3D, const float* shs, const float* colors_precomp,
                           const float* opacities, const float* scales, const float* rotations,
                           const float* cov3D_precomp, const int32_t* radii,
                           const float* out_color, const float* out_depth, const float* out_alpha,
                           const float* dL_dout_color, const float* dL_dout_depth,
                           const float* dL_dout_alpha,
                           const void* geom, const void* bin, const void* img,
                           const hgs_status* status, int64_t entry_capacity, void* bwd_scratch,
                           float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                           float* dL_dcolors_precomp, float* dL_dopacities, float* dL_dscales,
                           float* dL_drotations, float* dL_dcov3D_precomp,
                           void* const* stage_events, int32_t activation_flags, void* stream);

/* ---- backward: replaces _C.rasterize_gaussians_backward ----------------------------
 * `status` is a HOST copy of what hgs_forward reported (read after the stream has passed
 * the forward), or NULL: then nothing about the forward's result is needed on the host -
 * the blend backward is launched with the capacity-derived upper bound of workgroups
 * (entry_capacity/64 + tiles) and every kernel reads the device-side status (an
 * overflowed forward yields all-zero gradients).  `entry_capacity` must equal the value
 * given to hgs_forward (it fixes the carve of `bin`); so must the HGS_ANTIALIAS bit of the *_act
 * entry points (the backward recomputes the filter's factor from it), bwd_scratch must hold
 * hgs_bwd_scratch_bytes(num_rendered) - or (entry_capacity) when status is NULL - or, when
 * status->num_pairs is non-zero, hgs_bwd_scratch_bytes_pairs(num_rendered, status->num_pairs):
 * status->num_pairs DECLARES how many pair rows the scratch holds (0 = the worst case of 16 per
 * entry).  The kernels compare it with the count the forward left on the device; if the device
 * holds more pairs than declared (a stale or foreign status) no pair row is written and every
 * gradient of the call is NaN - loud, and in bounds (ABI v14; up to v13 this overran the scratch).
 * out_* are the forward's outputs (unmodified), dL_dout_* the incoming
 * gradients (any of them may be NULL = zeros).  Every dL_d* output that is non-NULL is
 * fully overwritten (no pre-zeroing needed, no atomics: results are deterministic);
 * dL_dmeans2D is (P,3) in NDC units with z = 0. */
int hgs_backward(const hgs_settings* s, int32_t P, int32_t M,
                 const float* means3D, const float* shs, const float* colors_precomp,
                 const float* opacities, const float* scales, const float* rotations,
                 const float* cov3D_precomp, const int32_t* radii,
                 const float* out_color, const float* out_depth, const float* out_alpha,
                 const float* dL_dout_color, const float* dL_dout_depth,
                 const float* dL_dout_alpha,
                 const void* geom, const void* bin, const void* img,
                 const hgs_status* status, int64_t entry_capacity, void* bwd_scratch,
                 float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                 float* dL_dcolors_precomp, float* dL_dopacities, float* dL_dscales,
                 float* dL_drotations, float* dL_dcov3D_precomp,
                 void* const* stage_events, void* stream);

/* ---- frustum test: replaces _C.mark_visible ----------------------------------------
 * present[i] = 1 iff the view-space depth of means3D[i] exceeds 0.2. */
int hgs_mark_visible(const hgs_settings* s, int32_t P, const float* means3D,
                     uint8_t* present, void* stream);

/* Mean squared distance of every point to its 3 nearest neighbours (own index excluded,
 * duplicates count): replaces `simple_knn._C.distCUDA2(points)`, which the reference calls to
 * initialise the scales of a new cloud
 * (/root/reference/gaussiansplatting/scene/gaussian_model.py:20,134; gs_renderer.py:14,386-389;
 * kernel submodules/simple-knn/simple_knn.cu:147-183).  points: [P][3] fp32, mean_dist2: [P]. */
int hgs_knn_mean_dist2(int32_t P, const float* points, float* mean_dist2, void* stream);
/* The same result (the same three distances per point, exactly) in near-linear time: a uniform grid sized on the device
 * from the bounding box, counting sort of the points by cell, ring search around each point's cell - the role of the
 * Morton sort + 1024-point box pruning of simple_knn.cu:63-221, without a global sort and without the two host round
 * trips of SimpleKNN::knn (:187-197).  `scratch`: hgs_knn_scratch_bytes(P) bytes (~28 B per point + 8 B per cell).
 * Degenerate clouds (more than 4096 points in one cell) take the brute force above; the choice is made on the device.
 * 100k points: ~2.5 ms -> tens of us; 5 M points (a densified avatar): ~6 s -> ms. */
size_t hgs_knn_scratch_bytes(int32_t P);
int hgs_knn_mean_dist2_grid(int32_t P, const float* points, float* mean_dist2, void* scratch, void* stream);

/* View-parallel reduction behind the single all-gather (the serial accumulation it
 * reproduces: /root/reference/threestudio/systems/GaussianDreamer.py:253-256,385-391).
 * gathered: [world][P][F] fp32 packs (per-Gaussian gradient columns, radii as the LAST column);
 * out: [P][F] = sum over ranks in rank order for columns < F-1, max for column F-1. */
int hgs_reduce_view_packs(int32_t world, int64_t P, int32_t F, const float* gathered, float* out,
                          void* stream);
/* The same as one link of a CHAIN of collectives (several views per rank, one collective per round of views, each
 * overlapped with the render of the next round): out = ((acc_in + rank 0) + rank 1) + ... in exactly that order (max on
 * the radii column), so that the chain over the rounds equals the serial accumulation over the views in view order
 * (/root/reference/threestudio/systems/GaussianDreamer.py:244-266,385-391) bit for bit.  acc_in may be NULL (= the call
 * above) and may alias out. */
int hgs_reduce_view_packs_acc(int32_t world, int64_t P, int32_t F, const float* gathered, const float* acc_in,
                              float* out, void* stream);

/* Packs one rank's contribution for that all-gather: out[P][15 + 3M] =
 * [dL/dmeans3D 3 | dL/dmeans2D 3 | dL/dsh 3M | dL/dopacity 1 | dL/dscale 3 | dL/drot 4 | radii 1]. */
int hgs_pack_view_contribution(int32_t P, int32_t M, const float* g_means3D, const float* g_means2D,
                               const float* g_sh, const float* g_opac, const float* g_scales,
                               const float* g_rot, const int32_t* radii, float* out, void* stream);

/* v15: the view-parallel step without its pack pass and without its unpack kernels.
 * hgs_backward_batch_packed = hgs_backward_batch_act whose per-Gaussian kernel writes the gradients of Gaussian i as ONE
 * row of `pack` [P][15 + 3M] in the layout above (dL/dmeans2D summed over the call's B views in view order, radii = max
 * over the views, as an exact fp32 integer) instead of six tensors that hgs_pack_view_contribution would read back and
 * interleave (7.2 MB written + read + written per 100k Gaussians on the exposed path of a step: the pack IS what the
 * rank sends).  SH + scale / rotation inputs only (the configuration the reference trains: gaussian_renderer/__init__.py:
 * 57-82 with both pipe flags off); dL_dmeans2D_views [B][P][3] is optional (NULL: not written).  Same status / scratch
 * rules as hgs_backward*.
 * hgs_reduce_view_packs_unpack = hgs_reduce_view_packs_acc (acc_in may be NULL) whose result goes straight into the six
 * gradient tensors + radii [P] int32 (the step's LAST reduction: no [P][F] intermediate, no slicing / rounding kernels). */
int hgs_backward_batch_packed(const hgs_settings* views, int32_t B, int32_t P, int32_t M, const float* means3D,
                              const float* shs, const float* opacities, const float* scales, const float* rotations,
                              const int32_t* radii, const float* out_color, const float* out_depth, const float* out_alpha,
                              const float* dL_dout_color, const float* dL_dout_depth, const float* dL_dout_alpha,
                              const void* geom, const void* bin, const void* img, const hgs_status* status,
                              int64_t entry_capacity, void* bwd_scratch, float* pack, float* dL_dmeans2D_views,
                              void* const* stage_events, int32_t activation_flags, void* stream);
int hgs_reduce_view_packs_unpack(int32_t world, int64_t P, int32_t M, const float* gathered, const float* acc_in,
                                 float* g_means3D, float* g_means2D, float* g_sh, float* g_opac, float* g_scales,
                                 float* g_rot, int32_t* radii, void* stream);

/* ---- bookkeeping either side of the path ------------------------------
 * Densification statistics of one training step over B views
 * (/root/reference/threestudio/systems/GaussianDreamer.py:253-256,289,385-391 and
 * gaussiansplatting/scene/gaussian_model.py:434-438), one pass:
 *   radii_max = max_b radii[b];  visible = radii_max > 0 (&& keep[i] if keep != NULL);
 *   g = sum_b dL_dmeans2D[b] (view order);  for visible Gaussians:
 *   max_radii2D = max(max_radii2D, radii_max), xyz_gradient_accum += |g.xy|, denom += 1.
 * dL_dmeans2D [B][P][3], radii [B][P]; accum / denom / max_radii2D [P] fp32 updated in place;
 * radii_max [P] int32 and visibility [P] uint8 are optional outputs. */
int hgs_densify_stats(int32_t B, int32_t P, const float* dL_dmeans2D, const int32_t* radii, const uint8_t* keep,
                      float* xyz_gradient_accum, float* denom, float* max_radii2D, int32_t* radii_max,
                      uint8_t* visibility, void* stream);

/* Clone / split / prune masks (gaussian_model.py:359-438): grad = accum / denom (NaN -> 0),
 * big = max scale > percent_dense * extent;  clone = grad >= thr && !big;  split = grad >= thr && big;
 * prune = opacity < min_opacity || (max_screen_size > 0 && (max_radii2D > max_screen_size ||
 * max scale > 0.1 * extent)) || (size_thresh > 0 && max scale > size_thresh)  [prune_only: size_thresh].
 * scales [P][3] / opacity [P] may be the RAW parameters (log-scale / logit; flags) - the activations are
 * fused.  Masks are uint8 [P] (any may be NULL); counts (3 x uint32, optional) receives the number of
 * set clone / split / prune bits. */
int hgs_densify_masks(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scales,
                      int32_t scales_are_log, const float* opacity, int32_t opacity_is_logit,
                      const float* max_radii2D, float grad_threshold, float percent_dense, float extent,
                      float min_opacity, float max_screen_size, float size_thresh, uint8_t* clone_mask,
                      uint8_t* split_mask, uint8_t* prune_mask, uint32_t* counts, void* stream);

/* Stable compaction for the pruning of every parameter tensor and both Adam moments
 * (gaussian_model.py:283-337): hgs_compact_index turns keep[P] into the list of kept source rows
 * (order preserved) and their number; hgs_gather_rows then moves any [P][row_floats] fp32 tensor. */
size_t hgs_compact_scratch_bytes(int32_t P);
int hgs_compact_index(int32_t P, const uint8_t* keep, int32_t* src_of_dst, uint32_t* num_kept, void* scratch,
                      void* stream);
int hgs_gather_rows(int64_t n_out, int32_t row_floats, const int32_t* src_of_dst, const float* src, float* dst,
                    void* stream);

/* Re-anchoring of the Gaussians on a posed mesh (/root/reference/animation.py:384-403, a numpy pass on the
 * CPU plus an H2D copy per frame there): xyz[i] = uvw[i] . (v0,v1,v2) + dist[i] * unit normal of face
 * mapping_face[i].  vertices [V][3] fp32, faces [F][3] int32, mapping_* [P]. */
int hgs_reanchor(int32_t P, const float* vertices, const int32_t* faces, const int32_t* mapping_face,
                 const float* mapping_uvw, const float* mapping_dist, float* xyz, void* stream);

/* Re-anchoring that also carries the Gaussians' rotations with their anchor faces (v17, additive; opt-in: beyond the
 * reference, which moves xyz only).  Quaternions are (w, x, y, z); R(q) is the reference's build_rotation
 * (gaussiansplatting/utils/general_utils.py:78-99) of q / |q|; p (x) q is the Hamilton product, R(p (x) q) = R(p) R(q).
 * Frame of a face with vertices a, b, c:
 *   e1 = (b - a) / |b - a|,  n = (b - a) x (c - a) / |(b - a) x (c - a)|,  e2 = n x e1,  F = [e1 e2 n] (columns);
 *   r(a, b, c) = a unit quaternion of F, converted from the largest of the four diagonal terms 1 +- F00 +- F11 +- F22 (no
 *   branch divides by a small number); its sign is unspecified and nothing downstream depends on it.
 *   r = (1, 0, 0, 0) if |b - a|^2 < 1e-30, |(b - a) x (c - a)|^2 < 1e-30, or either is not finite: a NaN or Inf vertex
 *   never puts a NaN into a rotation (the position of such a row is whatever hgs_reanchor gives).
 * bind != 0 (once per avatar, `vertices` = the rest mesh):  rot_out[i] = conj(r(face of i)) (x) rot_in[i];  xyz may be NULL
 *   (written like hgs_reanchor where given).
 * bind == 0 (every frame, `vertices` = the posed mesh):     rot_out[i] = r(face of i) (x) rot_in[i],  rot_in = what the
 *   bind call returned;  xyz[i] = hgs_reanchor's value, bit for bit (same expressions, same order).
 * rot_in is the RAW rotation parameter (not normalised): the products with unit quaternions keep its length, the caller's
 * activation normalises as always.  All arithmetic is fp32, each operation rounded, no contraction.  Scales and colours are
 * not re-posed.  rot_in / rot_out [P][4] fp32, the rest as hgs_reanchor.  P == 0: HGS_OK without a launch; P < 0 or a NULL
 * required pointer with P > 0: HGS_EINVAL. */
int hgs_reanchor_rot(int32_t P, const float* vertices, const int32_t* faces, const int32_t* mapping_face,
                     const float* mapping_uvw, const float* mapping_dist, const float* rot_in, int32_t bind, float* xyz,
                     float* rot_out, void* stream);

/* ---- the optimizer step: Adam over every parameter tensor of the model in ONE launch -------------------------------
 * The reference builds torch.optim.Adam over six groups of one tensor each (gaussiansplatting/scene/gaussian_model.py:
 * 156-165): a chain of elementwise kernels per group and step.  hgs_adam_step updates up to HGS_ADAM_MAX_TENSORS tensors
 * in one launch; the struct below travels by value as the kernel's argument (no device-side table, no H2D copy).
 * Per tensor: param / exp_avg / exp_avg_sq (updated in place) and grad, fp32, contiguous, rows x row_floats elements, and
 * the fp32 scalars the HOST derives in double from the group's lr, betas, eps and the step count t (after its increment):
 *   step_size = lr / (1 - beta1^t),  bc2_sqrt = sqrt(1 - beta2^t),  w1 = 1 - beta1,  beta2,  w2 = 1 - beta2,  eps.
 * Per element, each operation rounded to fp32 in this order (no contraction):
 *   m = m + (g - m) * w1;   v = v * beta2 + (g * g) * w2;   d = sqrtf(v) / bc2_sqrt + eps;   p = p - step_size * (m / d)
 * (torch.optim.Adam's non-fused, non-capturable step without weight decay, amsgrad or maximize).
 * visible (optional, uint8 [visible_rows]): only elements of rows r with visible[r] != 0 are touched; the param, exp_avg
 * and exp_avg_sq of every other row keep their bits.  Every tensor of the call must then have visible_rows rows
 * (HGS_ESHAPE otherwise).  The scalars stay those of the global step count.
 * Tensors whose four pointers are 16-byte aligned move in 16-byte accesses, others element by element (same values).
 * block_start is filled by hgs_adam_step (the caller's content is ignored).
 * Returns HGS_EINVAL for args == NULL, num_tensors outside [0, HGS_ADAM_MAX_TENSORS], negative rows / row_floats or a NULL
 * pointer of a tensor that has elements; zero tensors or zero elements: HGS_OK without a launch. */
#define HGS_ADAM_MAX_TENSORS 16
typedef struct hgs_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t rows;
  int32_t row_floats;
  float step_size, bc2_sqrt, w1, beta2, w2, eps;
} hgs_adam_tensor;
typedef struct hgs_adam_args {
  int32_t num_tensors;
  int64_t visible_rows;          /* read only when visible != NULL */
  const uint8_t* visible;
  hgs_adam_tensor t[HGS_ADAM_MAX_TENSORS];
  uint32_t block_start[HGS_ADAM_MAX_TENSORS + 1];   /* workgroups of tensor k: [block_start[k], block_start[k + 1]) */
} hgs_adam_args;
int hgs_adam_step(const hgs_adam_args* args, void* stream);

/* ---- posing a skinned body: linear blend skinning (the reference's per-frame SMPL-X forward) --------------------------
 * /root/reference/animation.py:552-556 -> load_smplx (:273-330) runs the `smplx` package's forward on the CPU for every
 * frame, copies the vertices to numpy and recentres / rescales them (:320-330).  [UPSTREAM-KNOWLEDGE] the computation is
 * that package's lbs(); it is not in the reference tree.  hgs_lbs_pose poses F frames of one body in two launches.
 * Sizes: V vertices; J joints (1 <= J <= HGS_LBS_MAX_JOINTS) with parents[0] = -1 and parents[j] < j (the HOST's check: the
 * kernels trust it, a broken table leaves joints at their local transform but reads nothing out of bounds);
 * K = 9 (J - 1) rows of pose blend shapes, or K = 0 for a body without them; F frames.
 * Per frame, every operation rounded to fp32 (no contraction), 3-term dot products as (a0 b0 + a1 b1) + a2 b2:
 *   - R_j from the axis-angle a_j = poses[f][j]: angle = |a + 1e-8|, k = a / angle, R = I + sin(angle) [k]x +
 *     (1 - cos(angle)) [k]x^2 (the package's batch_rodrigues: a zero pose gives R = I exactly, never a NaN);
 *   - pf = concat over j >= 1 of (R_j - I), row-major;  v_posed = v_shaped + sum_k pf[k] posedirs[k];
 *   - G_0 = [R_0 | J_0], G_j = G_parent [R_j | J_j - J_parent];  posed joint j = G_j.t;  A_j = [G_j.R | G_j.t - G_j.R J_j];
 *   - v = sum over the vertex's weight list, in list order, of w (A_j.R v_posed + A_j.t);
 *   - vertices[f][v] = ((v + transl[f]) - centre) * scale, joints[f][j] = ((G_j.t + transl[f]) - centre) * scale.
 * The sum over k is partitioned: row k belongs to slice k mod 32; a slice adds its rows in ascending k, the 32 slice sums
 * are added in a fixed tree.  No atomics: a call is bit-reproducible, and frame f of a call with F > 1 has the bits of a
 * call with that frame alone (frames are taken in tiles of HGS_LBS_FRAME_TILE, which share every load of posedirs).
 * Arrays: v_shaped [V][3], J_rest [J][3], parents [J] int32, poses [F][J][3], transl [F][3] or NULL, vertices [F][V][3]
 * (out), joints [F][J][3] (out) or NULL.
 * posedirs [K][posedirs_stride] fp32: row k holds the 3 V values of blend shape k, then padding; posedirs_stride is a
 * multiple of 4 and >= 12 ceil(V / 4), the pointer 16-byte aligned (every lane loads 16 bytes).  The padding is read
 * and ignored.  posedirs may be NULL when K = 0.
 * Skinning weights: the dense V x J matrix packed on the host into weight_width slots per vertex, weight_joint
 * [V][weight_width] int32 and weight_value [V][weight_width] fp32, joints ascending, unused slots (joint 0, weight 0);
 * 1 <= weight_width <= J (the most non-zeros of any vertex: nothing is dropped).  A joint index outside [0, J) is
 * clamped into it.
 * workspace: hgs_lbs_workspace_bytes(J, F) bytes (0 for J or F out of range), 16-byte aligned; after the call it holds
 * A [F][J][12] (rows of [R | t]), the posed joints [F][J][3] before transl and the affine, and pf [F][9 (J - 1)].
 * Returns HGS_EINVAL without a launch for args == NULL, J outside [1, HGS_LBS_MAX_JOINTS], negative V or F, V > 2^29,
 * K other than 0 or 9 (J - 1), weight_width outside [1, J], a posedirs_stride or alignment other than the above, or a
 * NULL pointer for an array that has elements; F == 0 or V == 0: HGS_OK without a launch.
 * v17 gained these exports without a change of any earlier signature. */
#define HGS_LBS_MAX_JOINTS 64
#define HGS_LBS_FRAME_TILE 8
typedef struct hgs_lbs_args {
  int32_t V, J, F, K;
  int32_t weight_width;
  int32_t posedirs_stride;       /* floats per row of posedirs (read only when K > 0) */
  const float* v_shaped;
  const float* J_rest;
  const int32_t* parents;
  const float* posedirs;
  const int32_t* weight_joint;
  const float* weight_value;
  const float* poses;
  const float* transl;           /* or NULL */
  float centre[3];
  float scale;
  void* workspace;
  float* vertices;
  float* joints;                 /* or NULL */
} hgs_lbs_args;
size_t hgs_lbs_workspace_bytes(int32_t J, int32_t F);
int hgs_lbs_pose(const hgs_lbs_args* args, void* stream);

/* ---- pose-control images: B views of one skeleton in one launch (the reference's Skeleton.draw / humansd_draw) ---------
 * The reference's training step (threestudio/systems/GaussianDreamer.py:268-287) copies each view's mvp matrix to the
 * host, draws a skeleton map with cv2 on the CPU (threestudio/utils/poser.py:361-459, :8-49) and uploads the float image.
 * hgs_pose_draw draws all B views on the device.  This definition is the contract; it is NOT cv2 pixel for pixel (outline
 * pixels may differ: cv2 fills a fixed-point polygon, a 360-gon for an ellipse and a midpoint circle).
 * points [K][4] fp32 (homogeneous, already in the reference's swapped axes), mvp [B][4][4] fp32 row-major, occlusion [B]
 * uint8 or NULL (no view occluded).  K = 17 for HGS_POSE_HUMANSD, 18 for HGS_POSE_OPENPOSE.  Outputs: image [B][H][W][3]
 * (fp32 in [0, 1], or uint8 with uint8_out != 0), kp [B][K][3] fp32 (xs, ys, conf), records [B][R][8] int32 with
 * R = hgs_pose_records_bytes(style, 1) / 32 (16 or 35).  Every byte of the three is written exactly once (no atomics:
 * the caller may pass uninitialised storage and a call is bit-reproducible); view b has the bits of a call with it alone.
 * Projection (poser.py:365-369, :420-424), fp32 with every operation rounded once, m = mvp[b], p = points[k]:
 *   clip_c = fma(m[c][3], p3, fma(m[c][2], p2, fma(m[c][1], p1, m[c][0] * p0)));  ndc_c = clip_c / clip_3 (IEEE division);
 *   xs = (ndc_0 + 1) / 2 * H,  ys = (ndc_1 + 1) / 2 * W - x with H and y with W, as the reference has it; the pixel COLUMN
 *   is int(xs) and the ROW int(ys), truncated toward zero (cv2 points are (x = column, y = row)).
 * Occlusion (:373-389, :428-445), for a view whose flag is set, with z = ndc_2, nose n = 0 and (left ear, right ear,
 * left eye, right eye) = (el, er, yl, yr) = (3, 4, 1, 2) for HumanSD and (17, 16, 15, 14) for OpenPose:
 *   z[n] > z[el] and z[n] < z[er]:  er is hidden, and yr too if xs[yr] > xs[yl];
 *   else z[n] < z[el] and z[n] > z[er]:  el is hidden, and yl too if xs[yl] < xs[yr];
 *   else z[n] > z[el] and z[n] > z[er]:  n, yl and yr are hidden;  else nothing is.
 * A keypoint is UNUSABLE if xs or ys is not finite or exceeds 8191 in magnitude (w <= 0 puts a point far away); no limb
 * that touches one is drawn (the reference would raise in int() or let cv2 clip).  With |coordinate| <= 8191, pixels in
 * [0, 4096) and limb_width <= 32767: every difference is below 2^14, every dot and cross product of two below 2^29, so
 * 4 cross^2 < 2^60 and w^2 L < 2^59 - the integer tests below cannot overflow int64.
 * HGS_POSE_HUMANSD (draw_humansd_skeleton): conf = 1, or 0 for a hidden keypoint.  Limb (colour, a, b) of the table is
 *   drawn iff conf[a] > 0.3, conf[b] > 0.3, both are usable and the view's sum over k (in order, fp32) of
 *   (xs + ys) + conf is > 0 (np.sum(pose) > 0).  Record {1, Ax, Ay, Bx, By, w, 0, rgb}: the capsule around the segment
 *   between the truncated integer endpoints A and B covers pixel P iff 4 d^2(P, AB) <= w^2, exactly: with t = AP.AB,
 *   L = AB.AB:  t <= 0: 4 |AP|^2 <= w^2;  t >= L: 4 |BP|^2 <= w^2;  else 4 (AP x AB)^2 <= w^2 L.  (cv2.line of thickness w
 *   plus the reference's end circles of radius w / 2, which lie inside the capsule.)  w = limb_width.
 * HGS_POSE_OPENPOSE (Skeleton.draw): conf = mask = 0 <= xs < H and 0 <= ys < W and not hidden.  First a disc per
 *   masked-in keypoint i, record {2, cx, cy, 16, 0, 0, 0, rgb(colour[i])}: dx^2 + dy^2 <= 16.  Then limb i of the table
 *   iff both its keypoints are masked in, record {3, cx, cy, a, theta, 4, 0, rgb}: centre (int((X0 + X1) / 2),
 *   int((Y0 + Y1) / 2)), a = int(sqrt((Y0 - Y1)^2 + (X0 - X1)^2) / 2), theta = int(atan2(Y0 - Y1, X0 - X1) * (180 / pi)),
 *   all fp32.  With T[k] = lround(16384 cos(k degrees)) (csrc/pose_trig.h), C = T[theta mod 360], S = T[(theta - 90) mod
 *   360], u = dx C + dy S, v = dy C - dx S and b = 4 the pixel at (dx, dy) from the centre is inside iff |u| <= a 2^14,
 *   |v| <= b 2^14 and u^2 b^2 + v^2 a^2 <= a^2 b^2 2^28 (after the first two the third stays below 2^58; a = 0 leaves the
 *   pixels with u = 0).
 * A record of an element that is not drawn is all zeros.  The raster reads the records and nothing else: a pixel starts
 * at 0 and takes the records in order; 1 and 2 overwrite it with rgb, 3 blends every channel as cv2.addWeighted(canvas,
 * .4, cur, .6, 0) does on uint8, c <- (4 c + 6 k + 5) / 10 in integers (the exact (2 c + 3 k) / 5 is never on a tie).
 * rgb = r | g << 8 | b << 16.  Output: float32(v) / float32(255) correctly rounded, or v itself for uint8.
 * Tables: num_limbs = 0 takes the style's own (HumanSD: the reference's 16 limbs and int(255 c) of seaborn's 16-colour hls
 * palette; OpenPose: its 17 limbs and the controlnet_aux colours); else limb[i] = {colour index, a, b} for i < num_limbs <=
 * HGS_POSE_MAX_LIMBS with indices inside the style's K and HGS_POSE_MAX_COLOURS, colour[i] = {r, g, b}.
 * Returns HGS_EINVAL without a launch for args == NULL, a style other than the two, a K that does not fit the style,
 * B < 0 or > 65535, H or W outside [1, 4096], limb_width outside [1, 32767], a table out of range, or a NULL points / mvp /
 * image / kp / records with B > 0; B == 0: HGS_OK without a launch.
 * v17 gained these exports without a change of any earlier signature. */
#define HGS_POSE_OPENPOSE 0
#define HGS_POSE_HUMANSD 1
#define HGS_POSE_MAX_LIMBS 17
#define HGS_POSE_MAX_COLOURS 18
#define HGS_POSE_RECORD_INTS 8
#define HGS_POSE_MAX_DIM 4096
typedef struct hgs_pose_args {
  int32_t style;                 /* HGS_POSE_OPENPOSE or HGS_POSE_HUMANSD */
  int32_t B, K, H, W;
  int32_t limb_width;            /* HumanSD: the capsule's width w (the reference: int(10 H / 512)); OpenPose: >= 1, unused */
  int32_t uint8_out;             /* image is uint8 instead of fp32 */
  int32_t num_limbs;             /* 0: the style's own tables */
  const float* points;
  const float* mvp;
  const uint8_t* occlusion;      /* or NULL */
  void* image;
  float* kp;
  int32_t* records;
  int32_t limb[HGS_POSE_MAX_LIMBS][3];
  uint8_t colour[HGS_POSE_MAX_COLOURS][3];
} hgs_pose_args;
size_t hgs_pose_records_bytes(int32_t style, int32_t B);   /* 0 for an unknown style or B < 0 */
int hgs_pose_draw(const hgs_pose_args* args, void* stream);

/* ---- the step's guidance images and opacity losses (between render_views and the diffusion guidance) -------------------
 * The reference stacks the B views' colour and depth (threestudio/systems/GaussianDreamer.py:285-302), normalises the
 * depth per view and repeats it to three channels (:330-333), resizes both with F.interpolate(mode="bilinear",
 * align_corners=False) and casts them (threestudio/models/guidance/dual_branch_guidance.py:762-770), and adds two losses
 * on the depth (GaussianDreamer.py:359-366).  hgs_step_images_forward computes all of it in three launches,
 * hgs_step_images_backward its gradient with respect to render and depth in three more; nothing is read back.
 * Inputs: render [B][3][H][W] and depth [B][1][H][W], fp32, contiguous.  Both must be FINITE: a NaN or an Inf in either is
 * outside this contract (min / max and the tie masks below are not defined for them).  Output size (h, w) with
 * 1 <= h <= H and 1 <= w <= W: the same size or downsampling; upsampling is refused.
 * Definition, every operation in fp32 rounded once unless said otherwise:
 *   dmin[b], dmax[b] = min / max of depth[b] (:331-332, amin / amax);  g = max of depth over all views (:302, depths.max()).
 *   nd      = (depth - dmin[b]) / (dmax[b] - dmin[b] + 1e-10f)                                   (:333)
 *   rgb_out[b][c]        = resize(render[b][c]);   depth_out[b][0], [1], [2] = resize(nd[b]), the same bits three times:
 *                          two contiguous [B][3][h][w] images, what the VAE is handed.
 *   resize (torch's align_corners=False rule), per axis with in = H or W, out = h or w and scale = float(in) / float(out):
 *     src = scale * (dst + 0.5f) - 0.5f, raised to 0 if negative;  i0 = min(int(src), in - 1);  i1 = min(i0 + 1, in - 1);
 *     l = src - i0 clamped to [0, 1];  out = (1 - ly) ((1 - lx) v[y0][x0] + lx v[y0][x1]) + ly ((1 - lx) v[y1][x0] + lx v[y1][x1]).
 *     At 2:1 l = 0.5 everywhere and this is the 2 x 2 box mean; at 16:1 (rgb_as_latents, 1024 -> 64) only 2 x 2 of every
 *     16 x 16 inputs are read, as torch does.
 *   op = depth / (g + 1e-5f)                                                                     (:302)
 *   loss_sparsity = mean over B H W of sqrt(op^2 + 0.01f)                                        (:359-361)
 *   loss_opaque   = mean of (x - 1) log(1 - x) - x log(x),  x = min(max(op, 1e-3f), 1 - 1e-3f)   (:363-366: binary_cross_entropy
 *                   of the clamped opacity with ITSELF as the target)
 *   half_images != 0: the two images are fp16, the fp32 result rounded once to nearest-even.
 * The sums: every workgroup adds its pixels in a fixed order in fp32 and leaves one partial; one workgroup adds the
 * partials in a fixed order in fp64.  No floating-point atomics anywhere: forward and backward are bit-reproducible.
 * Backward: torch's autograd of the formulas above, for incoming gradients grad_rgb, grad_depth ([B][3][h][w], fp32 or
 * fp16 as half_images says) and grad_loss_sparsity, grad_loss_opaque (one fp32 each, DEVICE memory, read by the kernel).
 * A NULL gradient is absent (not a zero tensor).  In particular:
 *   - dmin, dmax and g carry gradient: every element equal to the extremum receives grad / count (amin, amax and max()
 *     all share evenly among ties; the counts are exact integers, written to tie_counts by the forward:
 *     [b] = #(depth[b] == dmin[b]), [B + b] = #(depth[b] == dmax[b]), [2 B] = #(depth == g));
 *   - binary_cross_entropy(x, x): the input's own gradient is 0 (as torch has it, (x - t) / (x (1 - x)) with t = x), the
 *     target's is (log(1 - x) - log x) / N, and it passes the clamp only where 1e-3f <= op <= 1 - 1e-3f;
 *   - an empty view (depth[b] all 0): dmax = dmin, the denominator is 1e-10f, nd = 0 exactly; the gradient through nd is
 *     scaled by 1e10 - large, finite, and what torch computes.
 * grad_render is written iff grad_rgb is given, grad_depth_in iff any of the other three is; every element once.
 * The forward's depth_min, depth_max, depth_global_max and tie_counts are inputs of the backward.
 * workspace: hgs_step_images_workspace_bytes(B, H, W, h, w) bytes, 16-byte aligned, scratch of ONE call (nothing in it
 * lives from the forward to the backward).  render, depth, the images and the gradients must be 16-byte aligned.
 * Both return HGS_EINVAL before any device work for args == NULL, B < 1 or > 65535, any size below 1, h > H, w > W, H or W
 * above HGS_SI_MAX_DIM, B H W >= 2^31, a NULL or misaligned pointer among those the call needs; the backward with all four
 * gradients NULL: HGS_OK without a launch.  hgs_step_images_workspace_bytes is 0 for sizes the calls refuse.
 * The reductions cut a view into chunks of HGS_SI_PIXELS_PER_WORKGROUP pixels (HGS_SI_PIXELS_PER_THREAD per lane, one
 * 16-byte load) and give it min(chunks, HGS_SI_PARTIALS_PER_VIEW) workgroups = partials.
 * v17 gained these exports without a change of any earlier signature. */
#define HGS_SI_PIXELS_PER_THREAD 4
#define HGS_SI_PIXELS_PER_WORKGROUP 1024
#define HGS_SI_PARTIALS_PER_VIEW 256
#define HGS_SI_MAX_DIM 32768
typedef struct hgs_step_images_args {
  int32_t B, H, W, h, w;
  int32_t half_images;              /* rgb_out, depth_out, grad_rgb and grad_depth are fp16 instead of fp32 */
  const float* render;              /* [B][3][H][W] (forward) */
  const float* depth;               /* [B][1][H][W] */
  void* workspace;
  void* rgb_out;                    /* [B][3][h][w] (forward, written) */
  void* depth_out;                  /* [B][3][h][w] (forward, written) */
  float* loss_sparsity;             /* [1] (forward, written) */
  float* loss_opaque;               /* [1] (forward, written) */
  float* depth_min;                 /* [B] written by the forward, read by the backward */
  float* depth_max;                 /* [B] likewise */
  float* depth_global_max;          /* [1] likewise */
  uint32_t* tie_counts;             /* [2 B + 1] likewise */
  const void* grad_rgb;             /* [B][3][h][w] or NULL (backward) */
  const void* grad_depth;           /* [B][3][h][w] or NULL */
  const float* grad_loss_sparsity;  /* [1] on the device, or NULL */
  const float* grad_loss_opaque;    /* [1] on the device, or NULL */
  float* grad_render;               /* [B][3][H][W], written iff grad_rgb */
  float* grad_depth_in;             /* [B][1][H][W], written iff any of the other three gradients is given */
} hgs_step_images_args;
size_t hgs_step_images_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t h, int32_t w);
int hgs_step_images_forward(const hgs_step_images_args* args, void* stream);
int hgs_step_images_backward(const hgs_step_images_args* args, void* stream);

/* ---- the photometric loss of image fitting: L1 + D-SSIM forward and backward, PSNR ----------------------------------------
 * The reference's second training loop (gaussiansplatting/train.py) scores a render against a photograph with
 *   loss = (1 - lambda) l1_loss(image, gt) + lambda (1 - ssim(image, gt))         (utils/loss_utils.py, lambda_dssim = 0.2)
 * and evaluates with the same two functions and psnr (utils/image_utils.py).  hgs_photometric_forward computes all of them
 * in two launches, hgs_photometric_backward the gradient with respect to `image` in one; nothing is read back.
 * Inputs: image (x below) and gt (y), both [B][C][H][W] fp32, contiguous, finite.  N = B C H W.
 * Definition, every operation in fp32 rounded once (the library is built with -ffp-contract=off) unless said otherwise:
 *   w[11] = HGS_PM_WINDOW: exp(-(i - 5)^2 / (2 1.5^2)) normalised to sum 1, the fp32 values the reference's gaussian()
 *           holds.  F(v)(p) = sum_j w[j] (sum_i w[i] v(p + (j - 5, i - 5))): rows first, then columns, taps added in ascending
 *           order from 0, v = 0 outside the plane (conv2d's zero padding of 5).  The reference multiplies by the 121
 *           products w[j] w[i] instead; the two differ by fp32 rounding only.
 *   mu1 = F(x), mu2 = F(y), s1 = F(x x) - mu1 mu1, s2 = F(y y) - mu2 mu2, s12 = F(x y) - mu1 mu2   (E[x^2] - mu^2, as _ssim has it)
 *   A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1 mu1 + mu2 mu2 + C1, B2 = s1 + s2 + C2,  C1 = 0.01^2, C2 = 0.03^2
 *   S = (A1 A2) / (B1 B2)                                       the SSIM map; it is not written out
 *   ssim_image[b] = mean of S over image b,  ssim = mean of S over everything,  l1 = mean |x - y|,
 *   sqerr[b C + c] = sum of (x - y)^2 over plane (b, c),  loss = weight_l1 l1 + weight_dssim (1.0f - ssim)
 *   psnr[r] = 20 log10(1 / sqrt(mse[r])), mse the fp32 mean of (x - y)^2 over image r (psnr_per_plane == 0, [B] values: the
 *           reference's view(shape[0], -1) of a 4-D input) or over plane r (psnr_per_plane != 0, [B C] values: the same
 *           rule on a 3-D input); log10 and sqrt in fp64, rounded once; +inf where the two are identical.
 * The sums: one workgroup per tile of HGS_PM_TILE_H x HGS_PM_TILE_W pixels of one plane adds its pixels in a fixed order in
 * fp32 and leaves one partial per sum; one workgroup then adds a plane's partials in fp64 - lane l of a wave takes partials
 * l, l + HGS_PM_FINISH_CHUNK, ... in order, then a fixed tree over the lanes - and the planes' sums in a fixed order.
 * No floating-point atomics: every result is bit-reproducible and does not depend on the order the workgroups ran in.
 * with_grad != 0: the forward also leaves three derivative maps of S in the workspace, per pixel q,
 *   dS/ds12 = 2 A1 / (B1 B2),   dS/ds1 = -S / B2,
 *   dS/dmu1 = 2 (mu2 (A2 - A1) + mu1 S (B1 - B2)) / (B1 B2)     (the total derivative: through s1 and s12 as well)
 * and that workspace is an input of the backward.  with_grad == 0 (metrics only) writes none and needs no room for them.
 * Backward: the window is symmetric, so the adjoint of the zero-padded filter is F itself:
 *   gs = ((grad_ssim - weight_dssim grad_loss) / B + grad_ssim_image[b]) / (C H W),   gl = (grad_l1 + weight_l1 grad_loss) / N
 *   grad_image(p) = gs (F(dS/dmu1)(p) + (2 x(p)) F(dS/ds1)(p) + y(p) F(dS/ds12)(p)) + gl sign(x(p) - y(p)),  sign(0) = 0
 * grad_loss, grad_l1, grad_ssim (one fp32 each) and grad_ssim_image ([B]) are DEVICE memory read by the kernel; a NULL one is
 * absent (0).  Where gs == 0 the filter is skipped (the term is 0).  gt receives no gradient.
 * workspace: hgs_photometric_workspace_bytes(B, C, H, W, with_grad) bytes, 256-byte aligned; 0 for sizes the calls refuse.
 * Both return HGS_EINVAL before any device work for args == NULL, B, C, H or W below 1, H or W above HGS_SI_MAX_DIM,
 * B C > 65535, N >= 2^31, or a NULL pointer among those the call needs; the backward with all four gradients NULL: HGS_OK
 * without a launch (grad_image is then not written).
 * v17 gained these exports without a change of any earlier signature. */
#define HGS_PM_TILE_H 32
#define HGS_PM_TILE_W 32
#define HGS_PM_FINISH_CHUNK 64
#define HGS_PM_WINDOW {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005528f, 0.266011715f, \
                       0.213005528f, 0.109360687f, 0.0360007733f, 0.00759875821f, 0.00102838012f}
typedef struct hgs_photometric_args {
  int32_t B, C, H, W;
  int32_t with_grad;                /* forward: write the derivative maps into the workspace */
  int32_t psnr_per_plane;           /* psnr has B C values (the 3-D shape rule) instead of B */
  float weight_l1, weight_dssim;    /* 1 - lambda and lambda, each rounded to fp32 by the caller */
  const float* image;               /* [B][C][H][W] */
  const float* gt;                  /* [B][C][H][W] */
  void* workspace;                  /* written by the forward; with_grad: read by the backward */
  float* loss;                      /* [1] (forward, written) */
  float* l1;                        /* [1] */
  float* ssim;                      /* [1] */
  float* ssim_image;                /* [B] */
  float* sqerr;                     /* [B C] */
  float* psnr;                      /* [B], or [B C] with psnr_per_plane */
  const float* grad_loss;           /* [1] on the device, or NULL (backward) */
  const float* grad_l1;             /* [1] on the device, or NULL */
  const float* grad_ssim;           /* [1] on the device, or NULL */
  const float* grad_ssim_image;     /* [B] on the device, or NULL */
  float* grad_image;                /* [B][C][H][W] (backward, every element written once) */
} hgs_photometric_args;
size_t hgs_photometric_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_grad);
int hgs_photometric_forward(const hgs_photometric_args* args, void* stream);
int hgs_photometric_backward(const hgs_photometric_args* args, void* stream);

/* ---- closest point and signed distance to a triangle mesh (the reference's `cubvh`) ----------------------------------
 * The per-avatar anchoring of /root/reference/animation.py:333-378:
 *   BVH = cubvh.cuBVH(vertices, faces); dist, face, uvw = BVH.signed_distance(points, return_uvw=True, mode="raystab")
 * vertices [V][3] fp32, faces [F][3] int32, points [P][3] fp32.  This definition is the contract (cubvh's sign test is
 * modelled on instant-ngp's ray stab; its exact directions are not reproduced):
 *   - face[i] = the face minimising the fp32 squared distance d2 from point i to the triangle, ties to the lowest index
 *     ((d2, face) in lexicographic order).  Faces whose fp32 cross(v1 - v0, v2 - v0) is exactly zero (or not finite, or
 *     with an index outside [0, V)) are skipped.  uvw[i] = barycentric weights of the closest point (Ericson's
 *     region-based closest point on a triangle: closest = u v0 + v v1 + w v2, each >= 0, sum 1), dist[i] = sqrt(d2).
 *   - a point with a non-finite coordinate (or no face to measure against) gets face -1, dist NaN, uvw 0.
 *   - HGS_MESH_RAYSTAB: rays from the point along +-d_i, the 32 Fibonacci-lattice directions z_i = 1 - (2i + 1) / 32,
 *     theta_i = 2 pi frac(0.6180339887 i + 0.1234).  The point is INSIDE iff all 64 rays hit a non-skipped face at t > 0
 *     (watertight test of Woop, Benthin and Wald 2013: a ray through a shared edge or vertex does not slip between the
 *     triangles); then dist is negated (positive = outside for an outward-wound mesh).  HGS_MESH_UNSIGNED: no sign.
 * The grid path and the brute force (grid == NULL) return bit-identical dist, face and uvw.
 *
 * The grid's size depends on the data and the library does not allocate or synchronise, so it is built in two steps:
 *   1. hgs_mesh_grid_plan writes the box, the grid dimensions and the number of (face, cell) references into `info`
 *      (DEVICE, one hgs_mesh_grid_info);
 *   2. the caller copies `info` to the host once per mesh, allocates hgs_mesh_grid_bytes(&info_host) bytes (0: the plan
 *      is unusable - more than 2^31 - 1 references, or not a plan) and calls hgs_mesh_grid_build with the same
 *      vertices and faces.  The grid holds its own copy of the triangles; queries reuse it.
 * hgs_mesh_query: grid = a built grid (then vertices / faces are not read) or NULL (brute force over all faces: O(P F),
 * and O(64 P F) for the sign).  uvw [P][3] may be NULL.  F == 0 with P > 0 is HGS_EINVAL.
 * v17 gained these exports without a change of any earlier signature. */
#define HGS_MESH_UNSIGNED 0
#define HGS_MESH_RAYSTAB 1
typedef struct hgs_mesh_grid_info {
  uint32_t bmin[3], bmax[3];  /* order-preserving integer images of the box of the finite vertices (the plan's own use) */
  int32_t dims[3];            /* cells per axis                                                                      */
  uint32_t ncells;            /* dims[0] * dims[1] * dims[2]                                                         */
  float origin[3];            /* low corner of the box                                                               */
  float cell;                 /* cell edge                                                                           */
  int32_t num_faces;          /* F of the plan                                                                       */
  int32_t reserved0;
  uint64_t num_refs;          /* (face, cell) references: every non-skipped face in every cell of its bounding box   */
} hgs_mesh_grid_info;
int hgs_mesh_grid_plan(int32_t V, const float* vertices, int32_t F, const int32_t* faces, hgs_mesh_grid_info* info,
                       void* stream);
size_t hgs_mesh_grid_bytes(const hgs_mesh_grid_info* info_host);
int hgs_mesh_grid_build(int32_t V, const float* vertices, int32_t F, const int32_t* faces,
                        const hgs_mesh_grid_info* info_host, void* grid, void* stream);
int hgs_mesh_query(int32_t P, const float* points, int32_t V, const float* vertices, int32_t F, const int32_t* faces,
                   const void* grid, int32_t mode, float* dist, int32_t* face, float* uvw, void* stream);

/* ---- density field of the Gaussians and its iso-surface (the reference's mesh extraction) ----------------------------
 * GaussianModel.extract_fields / extract_mesh of /root/reference/gs_renderer.py:240-361: a Python loop over 16^3 blocks
 * there, followed by `mcubes.marching_cubes` on the CPU.  This definition is the contract:
 *   - xyz [P][3], opacity [P] (ACTIVATED, in [0, 1]), scaling [P][3] (ACTIVATED standard deviations), rotation [P][4] (RAW
 *     quaternion r, x, y, z; normalised here).  A Gaussian is KEPT iff opacity > 0.005 (and its centre is finite).
 *   - center = (min + max) / 2 of the kept centres, extent = the box's largest side, scale = fp32(1.8 / extent) (the
 *     division in fp64, as the reference's Python float); n = (xyz - center) * scale and s = scaling * scale in fp32.
 *   - `axis` [resolution] fp32 holds the sample positions of every axis (the reference: torch.linspace(-1, 1, resolution)),
 *     cut into num_blocks runs of resolution / num_blocks samples.  Block b of an axis spans lo_b = axis[first of run] -
 *     grow .. hi_b = axis[last of run] + grow (fp32; the reference: grow = relax_ratio * 2 / num_blocks).  A kept Gaussian
 *     is listed in block (bx, by, bz) iff lo < n < hi STRICTLY on all three axes; it then contributes to every sample of the
 *     block and to no other sample.  resolution % num_blocks == 0, 1 <= num_blocks <= 32, resolution <= 2048,
 *     resolution / num_blocks <= 256 (HGS_EINVAL otherwise).
 *   - occ[x][y][z] = sum over the block's list, in ASCENDING Gaussian index, of opacity * exp(power), power = -1/2 d^T
 *     Sigma^-1 d, d = sample - n; a term with power > 0 contributes 0.  fp32 throughout, one fixed instruction sequence:
 *     the field is bit-reproducible from call to call (no floating-point atomics).
 *   - Sigma^-1 is built as R diag(1 / s^2) R^T, NOT by the reference's adjugate of Sigma = R S^2 R^T with
 *     1 / (det + 1e-24): the same matrix without the adjugate's cancellation (measured in fp32 against fp64 on an avatar
 *     cloud: 4e-5 relative on the field instead of 4e-4).  The reference's + 1e-24 is not reproduced; it would change the
 *     field by more than 1 % only where det Sigma = (s0 s1 s2)^2 < 1e-22, i.e. for Gaussians whose normalised scales have a
 *     geometric mean below 2e-4 - a hundredth of the sample spacing at resolution 128.  exp(power) is evaluated as
 *     exp2 of the form with log2(e) folded into the six coefficients.
 * The lists' size depends on the data and the library does not allocate or synchronise, so a field takes two calls:
 *   1. hgs_field_plan (scratch `plan`: hgs_field_plan_bytes) filters, reduces the box, writes one 10-float record and the
 *      reached block range per Gaussian, counts every block's list and writes `info` (DEVICE);
 *   2. the caller copies `info` to the host once, allocates hgs_field_list_bytes(&info_host) bytes (0: not a usable plan)
 *      and calls hgs_field_eval with the same `axis` and `plan`.  num_kept == 0 (or a box of extent 0, which leaves no
 *      finite normalised centre): every list is empty and the field is zero.
 * block_counts (optional, [num_blocks]^3 int32, x-major like occ): the length of every block's list.
 *
 * hgs_mc_*: marching cubes of a field [X][Y][Z] fp32 (z fastest).  What it shares with `mcubes.marching_cubes` is the
 * coordinates, the interpolation and the inside rule below - NOT the triangle list: the case table (csrc/mc_table.h) is
 * this project's own, so in cells with an ambiguous face or a loop of five or more edges the triangles (and their number)
 * may differ from mcubes', while the set of vertices is the same.  A field with a dimension of one sample has no cell and
 * yields nothing (no vertices either).  Vertices
 * in index coordinates ([0, X-1] x [0, Y-1] x [0, Z-1]), on the crossed grid edges at (threshold - f0) / (f1 - f0)
 * between the edge's two samples.  A sample is INSIDE iff value >= threshold (NaN: outside).  ONE vertex per crossed
 * grid edge, shared by the triangles around it; vertices in the memory order of the edges (by low grid point, then x, y, z
 * direction), triangles in the memory order of the cells, inside a cell in the order of csrc/mc_table.h.  Triangles are
 * wound so that their normals point from inside to outside (from high values to low): a closed surface around a
 * maximum has positive signed volume.  Two calls again: hgs_mc_count classifies and scans (scratch: hgs_mc_scratch_bytes;
 * X, Y, Z >= 1, X Y Z <= 2^28) and writes the sizes to `info` (DEVICE); the caller reads them, allocates vertices
 * [num_vertices][3] fp32 and triangles [num_triangles][3] int32 and calls hgs_mc_emit with the same field and scratch.
 * v17 gained these exports without a change of any earlier signature. */
typedef struct hgs_field_info {
  uint32_t bmin[3], bmax[3];  /* order-preserving integer images of the box of the kept centres (the plan's own use)   */
  float center[3];
  float extent;               /* largest side of the box                                                               */
  float scale;                /* fp32(1.8 / extent)                                                                    */
  uint32_t num_kept;
  int32_t num_gaussians;      /* P of the plan                                                                         */
  int32_t num_blocks;         /* per axis                                                                              */
  int32_t resolution;
  float grow;
  uint64_t num_refs;          /* (Gaussian, block) references = the sum of all list lengths                            */
} hgs_field_info;
size_t hgs_field_plan_bytes(int32_t P, int32_t num_blocks);
int hgs_field_plan(int32_t P, const float* xyz, const float* opacity, const float* scaling, const float* rotation,
                   int32_t resolution, int32_t num_blocks, const float* axis, float grow, void* plan,
                   hgs_field_info* info, void* stream);
size_t hgs_field_list_bytes(const hgs_field_info* info_host);
int hgs_field_eval(const hgs_field_info* info_host, const float* axis, const void* plan, void* lists, float* occ,
                   int32_t* block_counts, void* stream);

typedef struct hgs_mc_info {
  uint32_t num_vertices;
  uint32_t num_triangles;
} hgs_mc_info;
size_t hgs_mc_scratch_bytes(int32_t X, int32_t Y, int32_t Z);
int hgs_mc_count(const float* field, int32_t X, int32_t Y, int32_t Z, float threshold, void* scratch, hgs_mc_info* info,
                 void* stream);
int hgs_mc_emit(const float* field, int32_t X, int32_t Y, int32_t Z, float threshold, const void* scratch,
                const hgs_mc_info* info_host, float* vertices, int32_t* triangles, void* stream);

/* ---- the field at arbitrary points: density, outward normal and colour (vertex attributes of the extracted mesh) -------
 * An extension: the reference's extract_mesh stops at (vertices, faces).  hgs_fsample evaluates the field of hgs_field_*
 * at M points instead of at the grid samples, over the SAME per-block lists.  This definition is the contract:
 *   Inputs: `info_host`, `axis`, `plan` and `lists` of a field as hgs_field_eval was given them and left them; points
 *   [M][3] fp32; optionally colors [P][3] fp32, indexed by the ORIGINAL Gaussian index (P = the plan's num_gaussians).
 *   For a point q:
 *   1. n = (q - center) * scale in fp32, a subtraction then a multiplication (what the plan applies to a centre);
 *      normalized != 0: n = q untouched (the caller already has normalised coordinates, e.g. grid positions).
 *   2. a component of n that is not finite: every output of the point is 0.
 *   3. per axis g = (number of axis samples <= n_a) - 1, clamped to [0, resolution - 1]; the block is g / (resolution /
 *      num_blocks).  A point exactly on a grid sample belongs to that sample's block; a point outside the grid uses
 *      the edge block.  (`axis` ascending, as torch.linspace gives it.)
 *   4. over the block's list, in ASCENDING Gaussian index, with d = n - centre_i and e_i = exp(power_i) exactly as in the
 *      field (exp2 of the folded form; 0 where the form is > 0):
 *        density = sum o_i e_i                       - at a point that IS a grid sample: occ there, bit for bit
 *        G       = sum o_i e_i Sigma_i^-1 d          - minus the gradient of the density, up to the positive constant of
 *                                                      the folding: in the record's terms, proportional to
 *                  -(2A dx + B dy + C dz, B dx + 2D dy + E dz, C dx + E dy + 2F dz)
 *        normal  = G / |G|, or (0, 0, 0) where G is 0 or not finite.  |G| is formed after G is divided by its largest
 *                  component, so the squares neither underflow nor overflow: every normal is a unit vector or zero.  It
 *                  points from high density to low - the side the marching-cubes triangles face - and is the same in
 *                  world space (the normalisation is a uniform scale).
 *        color   = (sum o_i e_i c_i) / density, or (0, 0, 0) where density is 0.
 *      A block with an empty list: zeros.
 *   5. fp32 throughout; each point's sums are its own, one fixed instruction sequence: the outputs are bit-reproducible
 *      from call to call and do not depend on where the point stands in the input.  No floating-point atomics (the
 *      binning counts with integer atomics; a point's place in its bin changes no result).
 * density [M], normal [M][3], color [M][3]: each optional (NULL: not computed); color requires colors.
 * scratch: hgs_fsample_scratch_bytes(M, num_blocks) bytes (host arithmetic; 0 for M < 0 or num_blocks outside 1 .. 32).
 * No host wait.  HGS_EINVAL before any launch for args == NULL, M < 0, color without colors, an info that
 * hgs_field_list_bytes refuses, or a NULL among the pointers the call needs.  M == 0 launches nothing.  A plan without
 * list entries (num_refs == 0; `lists` may then be NULL) gives zeros.
 * v17 gained these exports without a change of any earlier signature. */
typedef struct hgs_fsample_args {
  const hgs_field_info* info_host;
  const float* axis;                /* [resolution] */
  const void* plan;
  const void* lists;
  int32_t M;
  int32_t normalized;               /* points are normalised coordinates already */
  const float* points;              /* [M][3] */
  const float* colors;              /* [P][3] or NULL */
  void* scratch;
  float* density;                   /* [M] or NULL */
  float* normal;                    /* [M][3] or NULL */
  float* color;                     /* [M][3] or NULL */
} hgs_fsample_args;
size_t hgs_fsample_scratch_bytes(int32_t M, int32_t num_blocks);
int hgs_fsample(const hgs_fsample_args* args, void* stream);

/* ---- area-uniform samples of a triangle mesh (the reference's trimesh.sample.sample_surface, on the device) -------------
 * This definition is the contract; tests/surface_sample_reference.py restates it in numpy.
 *
 * Table (hgs_surface_cdf).  For face f with fp32 vertices a, b, c widened to fp64: e1 = b - a, e2 = c - a, the cross
 * product component by component (cx = e1y e2z - e1z e2y, cy = e1z e2x - e1x e2z, cz = e1x e2y - e1y e2x),
 * area = 0.5 * sqrt((cx cx + cy cy) + cz cz), no contraction.  A non-finite area counts as 0; a face with a vertex index
 * outside [0, V) counts as 0 and its vertices are never read.  cdf [F + 1] fp64: cdf[0] = 0 and cdf[k], k = 1 .. F, the
 * areas of faces 0 .. k-1 summed in this fixed order: entry k of block b (1024 entries a block) is S_b + (the areas of
 * the block's entries in front of k, added left to right), S_0 = 0, S_b+1 = S_b + (block b's areas added left to right).
 * So the table never decreases, a face of area 0 repeats the entry in front of it bit for bit, and the table is the same
 * from call to call (no floating-point atomics).
 * A = cdf[F].  info (DEVICE, 16 bytes): A and the number of faces of positive area.  scratch:
 * hgs_surface_cdf_scratch_bytes(F) bytes.  1 <= F <= HGS_SURFACE_MAX_FACES, V >= 0.  No host wait.
 *
 * Samples (hgs_surface_sample, one launch, no host wait).  Sample i of a call has the global index g = offset + i (64 bits,
 * wrapping); nothing else of the call enters its result, so rows k .. k+m of a call are the rows of a call of m samples at
 * offset + k.
 *   words   x0..x3 = Philox4x32-10(counter = (g_lo, g_hi, 0, 0), key = (seed_lo, seed_hi)): multipliers M0 = 0xD2511F53,
 *           M1 = 0xCD9E8D57; a round: (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the
 *           key grows by (0x9E3779B9, 0xBB67AE85) between rounds.
 *   face    u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53 in fp64, t = u * A, face = the number of k in 1 .. F with
 *           cdf[k] <= t (clamped to F - 1; t < A, so the clamp never fires).  A face of area 0 is never chosen.
 *   uvw     k1 = x2 >> 8, k2 = x3 >> 8; if k1 + k2 > 2^24: k1 = 2^24 - k1, k2 = 2^24 - k2 (trimesh's fold);
 *           uvw = (2^24 - k1 - k2, k1, k2) * 2^-24: exact in fp32, each in [0, 1], their sum exactly 1.
 *   point   per axis (a u + b v) + c w in fp32, no contraction: the bits of hgs_reanchor with dist = 0.
 * points [N][3] fp32, face [N] int32, uvw [N][3] fp32: each optional (NULL: not written).  N == 0 launches nothing.
 * A == 0 (or not > 0): face = -1, uvw = 0 and NaN points for every sample.  cdf is the table hgs_surface_cdf left for
 * the same vertices and faces.  HGS_EINVAL before any launch for args == NULL, N < 0, V < 0, F outside
 * 1 .. HGS_SURFACE_MAX_FACES, or a NULL among vertices, faces, cdf.
 *
 * hgs_init_gaussians: the tensors GaussianModel.create_from_pcd builds from a cloud, in one launch.  points enter only
 * through dist2 [P] (hgs_knn_mean_dist2_grid of them); colors [P][3] or NULL (the reference's constant 0.5);
 * M = (max_sh_degree + 1)^2 >= 1.  Outputs, each optional:
 *   features_dc [P][1][3] = (c - 0.5f) / 0.28209479177387814f     features_rest [P][M-1][3] = 0
 *   scaling [P][3] = logf(sqrtf(d < 1e-7f ? 1e-7f : d)), d = dist2 (all three columns; a NaN stays a NaN)
 *   rotation [P][4] = (1, 0, 0, 0)     opacity [P][1] = the fp32 nearest to ln(0.1f / (1 - 0.1f))     max_radii2D [P] = 0
 * v17 gained these exports without a change of any earlier signature. */
#define HGS_SURFACE_MAX_FACES ((1 << 20) - 1)
typedef struct hgs_surface_info {
  double area;                      /* A = cdf[F]                                                                          */
  uint32_t num_positive;            /* faces of positive area: the ones a sample can fall on                               */
  uint32_t reserved;
} hgs_surface_info;
typedef struct hgs_surface_sample_args {
  int32_t V, F;
  const float* vertices;            /* [V][3] */
  const int32_t* faces;             /* [F][3] */
  const double* cdf;                /* [F + 1], of hgs_surface_cdf */
  int64_t N;
  uint64_t offset;
  uint64_t seed;
  float* points;                    /* [N][3] or NULL */
  int32_t* face;                    /* [N] or NULL */
  float* uvw;                       /* [N][3] or NULL */
} hgs_surface_sample_args;
size_t hgs_surface_cdf_scratch_bytes(int32_t F);
int hgs_surface_cdf(int32_t V, const float* vertices, int32_t F, const int32_t* faces, double* cdf, hgs_surface_info* info,
                    void* scratch, void* stream);
int hgs_surface_sample(const hgs_surface_sample_args* args, void* stream);
int hgs_init_gaussians(int64_t P, int32_t M, const float* colors, const float* dist2, float* features_dc,
                       float* features_rest, float* scaling, float* rotation, float* opacity, float* max_radii2D,
                       void* stream);

/* ---- mesh view: a forward triangle rasterizer for the body mesh (the reference's render_mesh_normal) ------------------
 * The reference's animation loop draws the posed SMPL-X mesh shaded with its vertex normals through nvdiffrast's rasterize
 * and interpolate (animation.py:558-601).  These entry points are the forward-only subset that needs: no autograd, no
 * antialias, no textures.  All arithmetic is fp32 with every operation rounded once (no contraction; 1 / x, a / b and sqrt
 * are the correctly rounded IEEE operations) or exact integer arithmetic, so a call is bit-reproducible and view b of a
 * batch has the bits of a call with it alone.  Float atomics are not used; integer atomics only count and hand out slots.
 * vertices [V][3] (vertex_stride = 0: one mesh for all views) or [B][V][3] (vertex_stride = 3 V), mvp [B][4][4] row-major,
 * faces [F][3] int32 (a face with an index outside [0, V) is dropped).
 * 1. Vertex stage, per (view, vertex), m = mvp[b]:  c_i = ((m[i][0] x + m[i][1] y) + m[i][2] z) + m[i][3];  invw = 1 / c_3;
 *    xs = ((c_0 invw) 0.5 + 0.5) (float)(W << 8), ys likewise with c_1 and H;  zw = c_2 invw;  x_fix = (int)rintf(xs) (8
 *    sub-pixel bits).  The vertex is VALID iff c_3 > 0, xs, ys and zw are finite and |xs|, |ys| < 2^23.  records[b][v] =
 *    {x_fix, y_fix, bits(zw), bits(invw)}, or {INT32_MIN, 0, 0, 0} for an invalid vertex.  Pixel (row r, column c) is sampled
 *    at (c 256 + 128, r 256 + 128); row 0 is y_ndc = -1 (nvdiffrast's convention, and the 3DGS camera's).
 * 2. Coverage, exact in int64 (|coordinate| <= 2^23: differences < 2^25, cross products < 2^51).  With u x v = u_x v_y - u_y v_x
 *    and a, b, c the fixed-point corners: area2 = (b - a) x (c - a).  A triangle with an invalid vertex or area2 == 0 is
 *    dropped; both windings are drawn.  s = sign(area2), A = s area2, E0 = s ((c - b) x (p - b)), E1 = s ((a - c) x (p - c)),
 *    E2 = A - E0 - E1.  The sample p is inside iff for every i: E_i > 0, or E_i == 0 and edge i owns its boundary: with
 *    d0 = s (c - b), d1 = s (a - c), d2 = s (b - a), edge i owns iff d_y > 0 or (d_y == 0 and d_x > 0).  A sample exactly on
 *    an edge two triangles share belongs to exactly one of them (with rows growing with y: a horizontal edge belongs to
 *    the triangle below it, any other edge to the triangle on its left - a quad on pixel centres owns its top row and its
 *    right column).  There is NO near-plane clipping: a triangle with a vertex at c_3 <= 0 is dropped (a difference from
 *    nvdiffrast).
 * 3. Fragment:  ia = 1 / (float)A,  b_i = (float)E_i ia (int64 -> fp32 rounds to nearest even);  z = (b0 zw_a + b1 zw_b) +
 *    b2 zw_c; the fragment is discarded unless -1 <= z <= 1.  A pixel's winner has the smallest z, ties go to the lower
 *    face index - whatever the order of the internal lists.  p_i = b_i invw_i, d = (p0 + p1) + p2, u = p0 / d, v = p1 / d
 *    (perspective-correct weights of corners 0 and 1, as nvdiffrast's).  rast[b][r][c] = {u, v, z, (float)(face + 1)};
 *    a pixel nothing covers is all zeros.
 * 4. Interpolate, C <= HGS_MESHVIEW_MAX_ATTR channels of attr [V][C] (attr_stride = 0) or [B][V][C] (attr_stride = V C):
 *    ((u a0) + (v a1)) + (((1 - u) - v) a2) with a_k the attribute at corner k of the face; zeros where the fourth component
 *    of rast is not a face index in [1, F].
 * 5. Vertex normals (animation.py:573-590): adj_start [V + 1], adj [adj_start[V]] is the vertex -> corner adjacency in CSR
 *    form, each entry 3 face + corner, ascending inside a vertex.  n = the sum, in that order, component by component, of
 *    cross(v1 - v0, v2 - v0) = (e1_y e2_z - e1_z e2_y, e1_z e2_x - e1_x e2_z, e1_x e2_y - e1_y e2_x) of the entries' faces (a
 *    gather: no atomics).  SAFE NORMALISE: dot = (n_x n_x + n_y n_y) + n_z n_z; (0, 0, 1) if dot <= 1e-20f (or NaN), else
 *    n / sqrtf(fmaxf(dot, 1e-20f)) component by component.
 * 6. shade_normals != 0 (render_mesh_normal; C must be 3): the interpolated value gets the same safe normalise, then
 *    (n + 1) 0.5.  In an image, pixels without a face are `background` in every channel.
 * Calls: hgs_meshview_normals writes normals [Bv][V][3] for the Bv = (vertex_stride ? B : 1) meshes.  hgs_meshview_plan
 * writes records and, into plan (hgs_meshview_plan_bytes(B, F, H, W) bytes), every triangle's box of 16 x 16 pixel tiles,
 * the tiles' counts and their exclusive scan (gridscan.h); *info (DEVICE, 32 bytes) receives the sizes and the number of
 * list entries.  The caller copies *info to the host - the one host read of a call, as the field and mesh index builders
 * have one - and allocates hgs_meshview_list_bytes(info_host) bytes (0 is valid: nothing is listed).  hgs_meshview_draw
 * fills the tiles' lists (it uses up the plan's cursors: one draw per plan) and draws, one workgroup per tile: with image == NULL it writes rast [B][H][W][4]; else image
 * [B][H][W][C] shaded from attr directly (rast may be NULL: no round trip) and rast as well if it is given.
 * hgs_meshview_interpolate reads rast_in [B][H][W][4] and writes image (zeros for pixels without a face; background is not
 * applied).  Limits: B in [0, 65535], H and W in [1, 4096], B V, B F and B tiles below 2^31, at most 2^31 - 1 list entries
 * (hgs_meshview_list_bytes returns (size_t)-1 beyond).  B == 0, or F == 0 for normals: HGS_OK without a launch.
 * Returns HGS_EINVAL for sizes outside these or a NULL pointer of an array that has elements.
 * v17 gained these exports without a change of any earlier signature. */
#define HGS_MESHVIEW_MAX_DIM 4096
#define HGS_MESHVIEW_TILE 16          /* pixels per tile edge: 256 threads, one pixel each */
#define HGS_MESHVIEW_LIST_BATCH 256   /* triangles of a tile's list staged through LDS at a time */
#define HGS_MESHVIEW_MAX_ATTR 8
typedef struct hgs_meshview_info {
  uint64_t num_refs;                /* (triangle, tile) list entries of the call */
  int32_t B, V, F, H, W;
  uint32_t reserved;
} hgs_meshview_info;
typedef struct hgs_meshview_args {
  int32_t B, V, F, H, W;
  int32_t C;                        /* attribute channels, 1..HGS_MESHVIEW_MAX_ATTR (draw with image, interpolate) */
  int32_t shade_normals;
  float background;
  int64_t vertex_stride;            /* floats between the views' meshes: 0 or 3 V */
  int64_t attr_stride;              /* floats between the views' attributes: 0 or V C */
  const float* vertices;
  const float* mvp;
  const int32_t* faces;
  const int32_t* adj_start;         /* normals */
  const int32_t* adj;
  const float* attr;
  const float* rast_in;             /* interpolate */
  int32_t* records;                 /* [B][V][4]: written by plan, read by draw */
  void* plan;
  void* lists;
  hgs_meshview_info* info;          /* DEVICE: written by plan */
  float* rast;
  float* image;
  float* normals;
} hgs_meshview_args;
size_t hgs_meshview_plan_bytes(int32_t B, int32_t F, int32_t H, int32_t W);   /* 0 for sizes the calls refuse */
int hgs_meshview_normals(const hgs_meshview_args* args, void* stream);
int hgs_meshview_plan(const hgs_meshview_args* args, void* stream);
size_t hgs_meshview_list_bytes(const hgs_meshview_info* info_host);
int hgs_meshview_draw(const hgs_meshview_args* args, const hgs_meshview_info* info_host, void* stream);
int hgs_meshview_interpolate(const hgs_meshview_args* args, void* stream);

/* ---- mesh cleaning and decimation (what follows marching cubes in the reference's extract_mesh) -------------------------
 * The reference (gs_renderer.py:333-361) calls kiui's clean_mesh and decimate_mesh, pymeshlab on the CPU.  pymeshlab's
 * isotropic remeshing, quadric edge collapse and non-manifold repair are NOT reproduced: floaters are removed by connected
 * components, the mesh is decimated by vertex clustering on a uniform grid.  This definition is the contract
 * (tests/mesh_clean_reference.py restates it in numpy); every result is independent of the order in which threads arrive
 * and the same from call to call.  vertices [V][3] fp32, faces [F][3] int32.
 *
 * A face with an index outside [0, V) is IGNORED everywhere below (it connects nothing, is counted nowhere, is never kept)
 * and counted in info->bad_faces.  A vertex with a coordinate that is not finite contributes to no box; in the clustering
 * grid and on the lattice it is clamped as hgs_grid_cell1 clamps (NaN -> 0).
 *
 * a. COMPONENTS.  Vertices are connected through the faces that share them (a face with a repeated index connects its
 *    vertices like any other).  labels[v] = the smallest vertex index of v's component; a vertex no face references is a
 *    component of its own.  Per component, at index L = its label (all other entries 0):
 *      comp_faces[L] = the number of its faces;
 *      comp_diag2[L] = (dx dx + dy dy) + dz dz in fp32, d = fp32(max - min) of its finite vertices per axis (integer atomics
 *                      on ordered float keys); 0 for a component without a finite vertex.
 *    Built as ROUNDS of launches: per face m = min of its three labels goes by atomicMin into the three labels and into
 *    the labels' own labels (the roots are hooked); then one pointer-jumping pass labels[v] = labels[labels[v]].  Labels
 *    only decrease; changed[r] (DEVICE) counts the waves that lowered a label in round r, and the labels are final after a
 *    round with changed[r] == 0.  The caller reads `changed` (every few rounds) and stops there; V + 1 rounds always suffice.
 * b. CLEAN.  D2 = the squared diagonal, computed as comp_diag2 is, of the box of ALL finite vertices.  p = min_d / 100.0f,
 *    thr = (p * p) * D2, all fp32.  A face is KEPT iff its three indices are distinct (and in range), comp_faces[L] >= min_f
 *    and NOT comp_diag2[L] < thr, L = the label of its vertices.  A vertex is kept iff a kept face references it.  Output:
 *    the kept vertices in ascending original index (vertex_src [V'] = their original indices, optional), the kept faces in
 *    original order, re-indexed.
 * c. DECIMATE by vertex clustering.  Box: lo = min, ext = fp32(max - min) per axis of the finite vertices, emax = the
 *    longest ext.  Grid of g cells per axis, 1 <= g <= HGS_MESHCLEAN_G_MAX: inv_h = (float)g / emax, the cell of a vertex =
 *    hgs_grid_cell1(x, lo, inv_h, g) per axis, its key (cz g + cy) g + cx (30 bits); the cell edge h = emax / (float)g is
 *    only reported.  surviving(g) = the faces whose three vertices lie in three different cells; hgs_meshclean_count adds
 *    surviving(g[k]) to counts[k] (DEVICE, zeroed by the caller) for up to three grids in one launch (g[k] < 1: skipped).
 *    CHOOSING g is the caller's bisection and nothing else: lo = 1, hi = G_MAX + 1; while hi - lo > 1: mid = (lo + hi) / 2,
 *    lo = mid if surviving(mid) <= target else hi = mid; g = lo.  surviving(1) = 0, so surviving(g) <= target always,
 *    although surviving is not monotone.  (mid, (lo + mid) / 2 and (mid + hi) / 2 in one launch are two steps of it.)
 *    NEW VERTICES: one per cell that a surviving face references, ordered by the smallest vertex index in the cell.  Its
 *    position is the mean of ALL input vertices in the cell on a lattice: per axis q = fminf(fmaxf(floorf((x - lo) * qs +
 *    0.5f), 0), 1048576) with qs = 1048576.0f / emax (fp32), summed in 64-bit integers (atomics) with the count n; then in
 *    fp64 m = (double)sum / (double)n and position = (float)((double)lo + m * ((double)emax / 1048576.0)).  No float atomics.
 *    NEW FACES: the surviving faces in original order, indices replaced by their cells' new vertices, orientation kept.
 *    Faces with the same three new vertices in any order or orientation are duplicates: the lowest original index stays.
 *    Both equivalence classes (cell -> lowest vertex, vertex set -> lowest face) are hash tables of a power-of-two capacity of
 *    at least twice the items, built by atomicCAS / atomicMin whose RETURNED values alone are used, looked up in a later
 *    launch, every probe loop bounded by the capacity; running into the bound sets info->error (the result is then void).
 * Calls (no call allocates or waits; `scratch` = hgs_meshclean_scratch_bytes(V, F) bytes, shared by all of them; `info`
 * DEVICE, 64 bytes, rewritten by each _begin):
 *   components: hgs_meshclean_begin (labels = identity, box, bad_faces) -> hgs_meshclean_rounds (n rounds, changed [n]
 *     DEVICE) until a round changed nothing -> hgs_meshclean_components (comp_faces, comp_diag2).
 *   clean: the components, then hgs_meshclean_clean_mark (the keep rule and the two compactions; info->num_vertices /
 *     num_faces) -> the caller copies *info to the host and allocates -> hgs_meshclean_clean_emit.
 *   decimate: hgs_meshclean_begin with labels == NULL -> hgs_meshclean_count per bisection launch -> hgs_meshclean_decimate_mark
 *     (g) -> copy *info, allocate -> hgs_meshclean_decimate_emit.
 * Limits: 0 <= V, F <= 2^29 (hgs_meshclean_scratch_bytes returns 0 beyond, the calls HGS_EINVAL).  V == 0 or F == 0 where
 * nothing is to do: HGS_OK without a launch.  HGS_EINVAL before any launch for args == NULL, sizes outside the limits, a
 * NULL pointer of an array the call uses, g outside [1, G_MAX], an info_host that holds an error, bad faces or counts
 * above V / F.  v17 gained these exports without a change of any earlier signature. */
#define HGS_MESHCLEAN_G_MAX 1024
#define HGS_MESHCLEAN_MAX_ITEMS (1 << 29)
#define HGS_MESHCLEAN_ERR_CELL_TABLE 1u   /* info->error bits: a probe loop ran into its bound */
#define HGS_MESHCLEAN_ERR_FACE_TABLE 2u
typedef struct hgs_meshclean_info {
  uint32_t bmin[3], bmax[3];        /* ordered-key images of the box of the finite vertices */
  uint32_t bad_faces;               /* faces with an index outside [0, V) */
  uint32_t error;                   /* HGS_MESHCLEAN_ERR_* */
  uint32_t num_vertices, num_faces; /* of the output (clean_mark, decimate_mark) */
  uint32_t reserved[6];
} hgs_meshclean_info;
typedef struct hgs_meshclean_args {
  int32_t V, F;
  const float* vertices;
  const int32_t* faces;
  void* scratch;
  hgs_meshclean_info* info;         /* DEVICE */
  int32_t* labels;                  /* [V] */
  int32_t* comp_faces;              /* [V] */
  float* comp_diag2;                /* [V] */
  int32_t min_f;                    /* clean_mark */
  float min_d;
  float* vertices_out;              /* emit: [info_host->num_vertices][3] */
  int32_t* faces_out;               /* emit: [info_host->num_faces][3] */
  int32_t* vertex_src;              /* clean_emit: [num_vertices], may be NULL */
} hgs_meshclean_args;
size_t hgs_meshclean_scratch_bytes(int32_t V, int32_t F);   /* 0 for sizes the calls refuse; grows with V and with F */
int hgs_meshclean_begin(const hgs_meshclean_args* args, void* stream);
int hgs_meshclean_rounds(const hgs_meshclean_args* args, int32_t rounds, uint32_t* changed, void* stream);
int hgs_meshclean_components(const hgs_meshclean_args* args, void* stream);
int hgs_meshclean_clean_mark(const hgs_meshclean_args* args, void* stream);
int hgs_meshclean_clean_emit(const hgs_meshclean_args* args, const hgs_meshclean_info* info_host, void* stream);
int hgs_meshclean_count(const hgs_meshclean_args* args, const int32_t* g, uint32_t* counts, void* stream);
int hgs_meshclean_decimate_mark(const hgs_meshclean_args* args, int32_t g, void* stream);
int hgs_meshclean_decimate_emit(const hgs_meshclean_args* args, const hgs_meshclean_info* info_host, void* stream);

/* Library / ABI version (bumped on any signature change). */
int hgs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HGS_RAST_H */
