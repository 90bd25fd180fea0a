/*
 * gpnerf_hip.h -- C ABI of the MI355X (gfx950) per-ray render path of GP-NeRF.
 *
 * This is the drop-in boundary for the reference's per-ray hot path
 * (libs/renders + libs/nerfheads).  The reference is pure Python: there is no
 * existing FFI; each entry point below names the reference function(s) it
 * replaces (paths relative to the reference root).  The library is loaded with
 * ctypes.CDLL by gp-nerf_amd/_lib.py; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer marked "device" is HBM memory owned by the caller and only
 *     borrowed for the call; "host" pointers are ordinary CPU memory;
 *   - entry points never allocate, never synchronise and never throw; kernels are
 *     enqueued on `stream` (a hipStream_t passed as void*, NULL = default stream);
 *   - return value: 0 on success, a negative GPNERF_E_* code otherwise;
 *     gpnerf_strerror() gives the text;
 *   - all arithmetic is fp32 (the reference's dtype); V = 3 source views and
 *     C = 32 feature channels are compiled in (rgb_fc's 96 = 3*32 inputs hard-wire
 *     them in the reference too: libs/nerfheads/trainhead.py:96,143).
 */
#ifndef GPNERF_HIP_H
#define GPNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPNERF_VIEWS 3
#define GPNERF_CH 32
#define GPNERF_LEVELS 4

#define GPNERF_OK 0
#define GPNERF_E_ARG (-1)      /* null pointer / bad size */
#define GPNERF_E_LAUNCH (-2)   /* hipLaunchKernel failed; see hipGetLastError */
#define GPNERF_E_DEVICE (-3)   /* not a gfx950 device / no device */

#define GPNERF_FOLD_FIRST_LEVEL 2   /* vol_folded / gpnerf_fold_volumes: the two coarse levels of the four */

/* flags of gpnerf_render_fused */
#define GPNERF_FLAG_NEG_RAY 1u     /* Projector(neg_ray=True): a sample is in front of a source view iff h_z < 0
                                      (BaseRender.py:317-320, demo_render.py:550-553).  The dense renderer pairs it with
                                      GPNERF_FLAG_FLIP_SAMPLES; the progressive renderer's integral never flips */
#define GPNERF_FLAG_FLIP_SAMPLES 16u /* raw2outputs(neg=True): rgb and sigma reversed along the ray before compositing, z not
                                      (BaseRender.py:86-88,101); rgb_in_map pairs the weights with the un-flipped rgb_in (:147) */
#define GPNERF_FLAG_EARLY_TERM 2u  /* a ray stops at the first sample at whose start its transmittance T < term_eps (not in the
                                      reference; everything dropped is bounded by term_eps, depth by term_eps * far).  With the
                                      workspace and at least one round of wavefronts the samples are walked in 16-sample segments,
                                      one launch each, the rays still alive re-packed 32 to a wavefront (same bits per ray in any
                                      ray order); otherwise a 32-ray tile stops once all its rays have */
#define GPNERF_FLAG_SPLIT_F16 8u   /* dense layers on f16 MFMA with every fp32 operand split into f16 hi + lo (three MFMAs per
                                      k-step, f32 accumulation): ~fp32 accuracy (1e-6 on rgb), 3/16 of the fp32 MFMA cost.
                                      Needs frame->head_blob_split; operands must stay below the f16 range (65504):
                                      GPNERF_FLAG_SPLIT_GUARD checks it */
#define GPNERF_FLAG_SPLIT_GUARD 32u /* with GPNERF_FLAG_SPLIT_F16: track the largest magnitude that becomes an MFMA operand in every
                                      32-ray tile (raw features, cross-view mean / variance, every activation); tiles in which it
                                      reaches the f16 range are rendered again by the fp32 form in a second launch of the same
                                      call, so the result never depends on the range of the data.  Needs the workspace
                                      (gpnerf_render_workspace_bytes) and frame->head_blob_ref */
#define GPNERF_FLAG_OCC_CULL 4u    /* the progressive renderer's per-sample rules (libs/renders/demo_render.py): grid coordinates
                                      with its literal voxel size 0.005 instead of frame->voxel (:87-95), a sample is evaluated
                                      only where the occupancy volume (frame->occ) interpolates to > 0 (:270-283), culled
                                      samples carry alpha = 0, colour is kept only where alpha > 1e-14 (:317,:329-341);
                                      ray_mask counts kept samples only.  With the workspace and no per-sample output (weights,
                                      raw) the keep decisions are made in a pass before the launch and the tiles are handed out
                                      longest first; same bits either way */

#define GPNERF_FLAG_REF_ORDER 64u   /* the fp32 form in the REFERENCE's arithmetic order even when the frame carries folded volumes:
                                      every dense layer as sgemm's chain (k ascending from zero, bias last) in the unscaled
                                      domain, x / 3 with IEEE rounding, multiply-then-add trilinear taps, no folded levels.
                                      On trained parameters it sits at the op-for-op CPU oracle's distance from the reference
                                      where the folded form is 5-10 x further.  Needs frame->head_blob_ref */

#define GPNERF_FLAG_NO_EXITS 128u   /* diagnostic: every layer of every sample is evaluated -- without the fp32 forms' bit-exact exits
                                      (the sigma feature layer in empty space; the colour branch run only for samples whose weight
                                      alpha * T is not zero; the sample loop ended where every ray's transmittance is exactly 0:
                                      GpnerfOutputs.step_stats) -- the A/B that shows they change no bit */
#define GPNERF_FLAG_SHARED_DEVICE 256u /* other processes' kernels share this device: no launch of this call waits for its own
                                      workgroups.  (By default a launch on the tile queue that lists its colour work lets its own
                                      wavefronts evaluate the list once they have no tile left, every wavefront reporting before any
                                      leaves: fine on a device the process has to itself -- one process per GPU -- or shares with
                                      kernels that end on their own, a deadlock hazard only against another tenant's kernel that
                                      waits the same way while holding compute units.  With this flag the list goes to a second
                                      kernel: the same bits, 1-10 % slower.) */
#define GPNERF_FLAG_RESERVE_CUS(n) (((uint32_t)(n) & 0xffu) << 24)
                                   /* bits 24..31: plan the launch for n fewer compute units (rounded down to a multiple of 8: one
                                      per XCD round).  The persistent workgroups then leave n CUs idle for kernels of other
                                      streams -- a pipelined evaluation loop runs the NEXT frame's encoder and volume builder
                                      there (an experiment of the pipelined evaluation loop: profiles/r05/d_pipeline.txt).  The maps are those of
                                      a chip with n fewer CUs: the same bits unless that makes the launch split tiles (see `workspace`) */

/* Per-frame constants (everything render_rays reads that does not depend on the ray).
 * Layouts are channels-last so that one bilinear / trilinear tap is one contiguous
 * 128-byte line; gpnerf_relayout_* produce them from the reference's NCHW tensors. */
typedef struct GpnerfFrame {
    const float* vol[GPNERF_LEVELS];        /* device; level k: [D_k][H_k][W_k][32]; SparseConvNet.py:111 `.dense()` */
    int32_t vol_dhw[GPNERF_LEVELS][3];
    const float* featmaps;                  /* device; [V][fh][fw][32]; encoder output, BaseRender.py:222 */
    int32_t feat_h, feat_w;
    const float* imgs;                      /* device; [V][H][W][4] = r,g,b,0 in [0,1]; BaseRender.py:231 */
    int32_t img_h, img_w;
    float proj[GPNERF_VIEWS][12];           /* rows 0..2 of K4 @ P4, row-major 3x4; BaseRender.py:233-247,314 */
    float Rh[9];                            /* batch['Rh'][0], row-major; BaseRender.py:52-60 */
    float Th[3];
    float bounds_min[3];                    /* batch['bounds'][0,0], SMPL-frame xyz; BaseRender.py:65 */
    float voxel[3];                         /* cfg.dataset.voxel_size (applied in d,h,w order); BaseRender.py:67 */
    int32_t out_sh[3];                      /* batch['out_sh'] d,h,w; BaseRender.py:69-70 */
    const float* head_blob;                 /* device or NULL (needed only by the folded form and gpnerf_fold_volumes);
                                               gpnerf_pack_head() image, gpnerf_head_blob_floats() floats */
    const float* head_blob_split;           /* device or NULL; gpnerf_pack_head_split() image (GPNERF_FLAG_SPLIT_F16) */
    const float* occ;                       /* device or NULL; [D_1][H_1][W_1] occupancy `masks3d` at level-1 size
                                               (SparseConvNet.py:135-139), read only with GPNERF_FLAG_OCC_CULL */
    const float* vol_folded[GPNERF_LEVELS]; /* device or NULL; levels GPNERF_FOLD_FIRST_LEVEL.. (all of them or none; the finer
                                               levels' entries are ignored): [D_k][H_k][W_k][64], written by gpnerf_fold_volumes
                                               from vol[] and head_blob.  With them the fp32 form of gpnerf_render_fused
                                               interpolates these levels' share of the sigma feature layer's pre-activation
                                               instead of running it per sample (same result up to fp32 rounding) */
    const float* head_blob_ref;             /* device or NULL; gpnerf_pack_head_ref() image: the fp32 form in the reference's
                                               summation order (GPNERF_FLAG_REF_ORDER, frames without vol_folded, and the
                                               fix-up launch of GPNERF_FLAG_SPLIT_GUARD) */
} GpnerfFrame;

/* The per-ray MLP parameters in PyTorch layout (weight [out][in] row-major, bias [out]),
 * host memory.  Names follow the reference state_dict. */
typedef struct GpnerfHeadParams {
    const float *geo_w, *geo_b;   /* sigmahead.out_geometry_fc.0  64x128 */
    const float *b1_w, *b1_b;     /* rgbhead.base_fc.0            64x105 */
    const float *b2_w, *b2_b;     /* rgbhead.base_fc.2            32x64  */
    const float *v1_w, *v1_b;     /* rgbhead.vis_fc.0             32x32  */
    const float *v2_w, *v2_b;     /* rgbhead.vis_fc.2             32x32  */
    const float *r1_w, *r1_b;     /* rgbhead.rgb_fc.0             32x96  */
    const float *r2_w, *r2_b;     /* rgbhead.rgb_fc.2             16x32  */
    const float *r3_w, *r3_b;     /* rgbhead.rgb_fc.4              3x16  */
    const float *d1_w, *d1_b;     /* rgbhead.out_geometry_fc.0    64x134 */
    const float *d2_w, *d2_b;     /* rgbhead.out_geometry_fc.2    32x64  */
    const float *d3_w, *d3_b;     /* rgbhead.out_geometry_fc.4    16x32  */
    const float *d4_w, *d4_b;     /* rgbhead.out_geometry_fc.6     1x16  */
} GpnerfHeadParams;

/* Outputs of Renderer.render_rays (BaseRender.py:148-156), all device, [N,...] row-major.
 * rgb/depth/acc/disp are required, the rest may be NULL. */
typedef struct GpnerfOutputs {
    float* rgb;        /* [N,3]  rgb_map   */
    float* depth;      /* [N]    depth_map */
    float* acc;        /* [N]    acc_map   */
    float* disp;       /* [N]    disp_map  */
    float* weights;    /* [N,S]  ret['alpha'] (= weights) */
    float* z_vals;     /* [N,S]  */
    float* rgb_in;     /* [N,9]  rgb_in_map (view-major, then rgb) */
    uint8_t* ray_mask; /* [N]    raw2outputs' mask: #samples with >1 valid view > 8 */
    float* raw;        /* [N,S,4] NeRFHead.forward output (rgb, sigma), un-flipped sample order */
    int32_t* samples_done; /* [N]  diagnostic: samples the ray's wavefront evaluated (S unless early termination / culling
                              skipped some); with it the launch never splits a tile's samples over several wavefronts */
    uint32_t* step_stats;  /* [8] or NULL, zeroed by the caller; the launch ADDS, per wavefront step of 32 samples:
                              [0] steps the launch answers for (sample-loop steps + [3]);
                              [1] steps without the sigma feature layer: all four volume levels exactly zero in all 32 samples
                                  (reference-order form: ELU(bias) without the layer's MFMAs), or counted in [3];
                              [2] [0] MINUS [5];
                              [3] steps settled BEHIND the sample loop, without a gather or an MFMA, because every ray's
                                  transmittance was exactly 0 (zero weights and the ray_mask count are all they still owe);
                              [4] volume LEVELS left out of the sigma feature layer (each a quarter of the layer; 0..4 per
                                  sample-loop step: a level whose 16 features are zero in all 32 samples adds fma(w, 0, s) = s);
                              [5] evaluations of the colour branch on 32 samples: one per step where it runs in the step, one
                                  per colour pass where it is deferred -- a sample whose weight alpha * T is exactly 0 adds
                                  fma(0, rgb, c) = c to the colour map, so only the samples that need it are evaluated, 32 at a
                                  time: listed for the launch as a whole where the workspace has room for the list (fp32 forms
                                  on the tile queue) and evaluated by the launch's own wavefronts once they have no tile left
                                  (launches on the tile queue with no remainder launch behind them) or by a second kernel (exactly ceil(listed / 32) evaluations),
                                  out of a queue per wavefront otherwise (never with `raw`, never under GPNERF_FLAG_NO_EXITS);
                              [6], [7] reserved (0).
                              All of it is bit-exact; bench.py prices its roofline on the work done:
                              sample-loop steps x (everything but the colour branch) - [4] x layer / 4 + [5] x colour branch */
} GpnerfOutputs;

/* Number of floats of the packed head image. */
int64_t gpnerf_head_blob_floats(void);

/* Re-arrange the PyTorch-layout parameters into the LDS image the kernels stage
 * (MFMA A-operand order).  Host-side, model-load time.
 * Replaces nothing in the reference; it is what load_state_dict is to nn.Linear. */
int gpnerf_pack_head(const GpnerfHeadParams* params_host, float* blob_host);

/* The same parameters for the reference-order fp32 form (GPNERF_FLAG_REF_ORDER): gpnerf_head_blob_floats() floats, rows and
 * columns in the order libs/nerfheads/trainhead.py's nn.Linear layers accumulate them on the CPU (sgemm), nothing pre-scaled. */
int gpnerf_pack_head_ref(const GpnerfHeadParams* params_host, float* blob_host);

/* The same parameters as f16 hi/lo pairs in v_mfma_f32_32x32x16_f16 A-operand order (GPNERF_FLAG_SPLIT_F16). */
int64_t gpnerf_head_blob_split_floats(void);
int gpnerf_pack_head_split(const GpnerfHeadParams* params_host, float* blob_host);

/* sigmahead.out_geometry_fc (trainhead.py:39-40,58) is linear in the 4 x 32 volume features, and F.grid_sample
 * (SparseConvNet.py:113-116) is linear in the voxels: Linear(sum_t w_t v_t) = sum_t w_t Linear(v_t).  For the coarse levels
 * k >= GPNERF_FOLD_FIRST_LEVEL this applies the layer's 32 columns of level k (without the bias) to every voxel of vol[k] --
 * once per frame instead of once per sample -- and writes 64 values per voxel in the order the sample loop accumulates them.
 * out: host array of GPNERF_LEVELS device pointers (entries below GPNERF_FOLD_FIRST_LEVEL unused), D_k * H_k * W_k * 64 floats. */
int gpnerf_fold_volumes(const GpnerfFrame* frame, float* const* out, void* stream);

/* Fused sample -> gather -> MLP -> composite over N rays.
 * Replaces Renderer.batchify_rays + render_rays with is_train=False
 * (libs/renders/BaseRender.py:110-184): get_sampling_points :35-50, pts_to_can_pts :52-60,
 * get_grid_coords :62-73, Projector.compute :326-363 (sample part), SparseConvNet.forward's
 * trilinear sampling (libs/nerfheads/networks/SparseConvNet.py:113-122),
 * NeRFSigmaHead.out_geometry_fc + NeRFRGBHead.forward (libs/nerfheads/trainhead.py:39-40,58,118-145)
 * and raw2outputs :75-107, rgb_in_map :147.
 *   rays: device [N][8] = origin(3), direction(3, un-normalised), near, far (BaseRender.py:250)
 *   term_eps: transmittance threshold, read only with GPNERF_FLAG_EARLY_TERM
 *   ray_order: optional device [N] list of distinct row indices (NULL = identity): launch slot i renders the ray in row
 *     ray_order[i] of `rays`; inputs are read and outputs written at that row, so results do not depend on the order.  In the
 *     plain case it is a permutation of 0..N-1; it may also pick N rows out of larger `rays` / output arrays (the progressive
 *     renderer passes every pixel's ray and the list of selected pixels: rows not listed are neither read nor written).
 *     It only decides which 32 rays share a wavefront and which 256 share a workgroup: pass image patches
 *     (e.g. 32x8 pixels per workgroup) so neighbouring rays hit the same cache lines.
 *   workspace: optional device scratch of gpnerf_render_workspace_bytes() bytes (NULL = none).  With it the launch balances
 *     its load: frames of more than one round of workgroups run as persistent workgroups that pull 32-ray tiles from a queue
 *     in the workspace (a tile's cost varies under early termination / culling; results are unchanged, bit for bit), and
 *     frames too small to fill the chip let 2, 4 or 8 wavefronts share the samples of one tile and merge their partial
 *     composites (second small launch); the transmittance product is then associated per segment, a ~1e-7 relative
 *     difference (never with GPNERF_FLAG_EARLY_TERM).  On the tile queue the fp32 forms also keep the LIST of the samples whose
 *     colour branch has to run there (32 bytes per sample of the launch: an entry and a result; launches of up to 2^26 samples)
 *     -- the sample loop then only lists them, the list is evaluated 32 entries per wavefront step, balanced whatever the rays
 *     (by the same launch's wavefronts as they run out of tiles, or by a second kernel: behind the segment launches of early
 *     termination, and always under GPNERF_FLAG_SHARED_DEVICE), and a last kernel adds every ray's terms in sample order: the colour map's bits are those of the loop
 *     that evaluates them in place, which is what a workspace too small for the list gets (gpnerf_render_workspace_bytes
 *     includes it).
 *     The workspace is private to the call until the stream reaches its end. */
int gpnerf_render_fused(const GpnerfFrame* frame, const float* rays, int64_t n_rays, int32_t n_samples,
                        uint32_t flags, float term_eps, const int32_t* ray_order, const GpnerfOutputs* out,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Bytes of workspace gpnerf_render_fused can use for this launch (0: it would not split); any smaller amount is valid -- the
 * launch keeps to the forms that fit. */
size_t gpnerf_render_workspace_bytes(int64_t n_rays, int32_t n_samples);
/* GPNERF_FLAG_SPLIT_GUARD keeps its state in the last gpnerf_render_guard_bytes(n_rays) bytes of the workspace (start rounded down
 * to 256): word 0 = number of flagged tiles once the stream has passed the call, words 64.. = one flag per 32-ray tile. */
size_t gpnerf_render_guard_bytes(int64_t n_rays);

/* What gpnerf_render_fused would do with a call, without touching a device: the launch plan and the workspace layout it derives
 * from the call's numbers alone.  A caller can ask what a workspace size buys before allocating it (does a 48 MB cap still list
 * the colour work?  does the frame take a remainder launch?), and the tests pin every plan down through it.  Host arithmetic only;
 * the same planner, argument checks and GPNERF_FLAG_RESERVE_CUS handling as the render call.
 *   n_rays, n_samples, flags, workspace_bytes: as for gpnerf_render_fused (workspace_bytes 0 = no workspace)
 *   n_cus: the device's compute units (hipDeviceProp_t::multiProcessorCount) BEFORE GPNERF_FLAG_RESERVE_CUS is taken off
 *   facts: GPNERF_PLAN_* bits -- the optional outputs the call asks for and what its frame carries
 * Returns GPNERF_E_ARG where the render call would (n_samples < 1, n_rays < 0 or >= 2^31, a guarded call without room for the
 * guard), and for n_cus < 1 or plan == NULL; n_rays == 0 gives an all-zero plan (nothing is launched). */
#define GPNERF_PLAN_WEIGHTS 1u        /* GpnerfOutputs.weights != NULL */
#define GPNERF_PLAN_RAW 2u            /* GpnerfOutputs.raw != NULL */
#define GPNERF_PLAN_SAMPLES_DONE 4u   /* GpnerfOutputs.samples_done != NULL */
#define GPNERF_PLAN_FOLDED 8u         /* the frame carries folded volumes that the render call accepts: GpnerfFrame.vol_folded set for
                                         all coarse levels, each below 2^32 bytes (256 per voxel) with x-rows below 2^24 bytes
                                         -- the render call ignores folded volumes beyond that and runs the reference-order form */
#define GPNERF_PLAN_OCC 16u           /* the frame carries an occupancy volume (GpnerfFrame.occ) */
/* sel: the arithmetic of the call */
#define GPNERF_SEL_REF 0              /* fp32, the reference's summation order */
#define GPNERF_SEL_FOLD 1             /* fp32, coarse levels folded */
#define GPNERF_SEL_SPLIT 2            /* GPNERF_FLAG_SPLIT_F16 */
#define GPNERF_SEL_GUARD 3            /* GPNERF_FLAG_SPLIT_F16 | GPNERF_FLAG_SPLIT_GUARD: the split form + the fp32 fix-up launch */
/* colour: where a sample's colour branch runs */
#define GPNERF_COLOUR_STEP 0          /* in the sample loop's step (GPNERF_FLAG_NO_EXITS, a `raw` output) */
#define GPNERF_COLOUR_WAVE 1          /* deferred to a queue per wavefront */
#define GPNERF_COLOUR_LIST 2          /* listed for the whole launch, evaluated by a second kernel */
#define GPNERF_COLOUR_UNIFIED 3       /* listed, evaluated by the listing launch's own wavefronts */
/* shape: the render launches */
#define GPNERF_SHAPE_STATIC 0           /* one launch, one unit per wavefront (`split` wavefronts share a tile's samples) */
#define GPNERF_SHAPE_QUEUE 1            /* persistent workgroups on the tile queue */
#define GPNERF_SHAPE_QUEUE_REMAINDER 2  /* the same over the first main_rays rays (whole rounds) + one launch over the rest */
#define GPNERF_SHAPE_REMAINDER_UNITS 3  /* one launch whose units are the whole round's tiles and the remainder's */
#define GPNERF_SHAPE_CHAINED 4          /* early termination: one launch per segment of samples */
#define GPNERF_PLAN_CLEARS 5
typedef struct GpnerfRegion { uint64_t off, bytes; } GpnerfRegion;   /* of the workspace; bytes == 0: not used by the call */
typedef struct GpnerfRenderPlan {
    int32_t sel, colour, shape;             /* GPNERF_SEL_* / GPNERF_COLOUR_* / GPNERF_SHAPE_* */
    int32_t waves, split;                   /* wavefronts per workgroup; wavefronts that share one tile's samples */
    uint32_t grid;                          /* workgroups of every render launch */
    int32_t n_cus, reserved_;               /* the compute units planned for (n_cus less GPNERF_FLAG_RESERVE_CUS) */
    int64_t tiles, main_rays;               /* 32-ray tiles of the call; launch slots of the first render launch */
    GpnerfRegion queue, part, chain, list, mask, guard;  /* tile-queue counters, split partials, early termination's chain block
                                               (its first control words are the queue's counters: the one overlap), colour list,
                                               cull mask + tile order, range guard */
    GpnerfRegion clear[GPNERF_PLAN_CLEARS]; /* what the call zeroes before its first launch */
} GpnerfRenderPlan;
int gpnerf_render_plan(int64_t n_rays, int32_t n_samples, uint32_t flags, int32_t n_cus, uint32_t facts, size_t workspace_bytes,
                       GpnerfRenderPlan* plan);

/* Stage entry points (the same device code as the fused kernel, one reference function per launch).
 *
 * get_sampling_points + pts_to_can_pts + get_grid_coords (libs/renders/BaseRender.py:35-73), jitter off:
 *   pts [N][S][3] world points, z_vals [N][S], grid [N][S][3] normalised volume coords (xyz); any may be NULL. */
int gpnerf_sample_points(const GpnerfFrame* frame, const float* rays, int64_t n_rays, int32_t n_samples, float* pts,
                         float* z_vals, float* grid, void* stream);
/* SparseConvNet.forward's F.grid_sample over the 4 dense levels
 * (libs/nerfheads/networks/SparseConvNet.py:113-122): grid [P][3] -> vol_feat [P][128] (level-major). */
int gpnerf_sample_volume(const GpnerfFrame* frame, const float* grid, int64_t n_points, float* vol_feat, void* stream);
/* Projector.compute for sample points (libs/renders/BaseRender.py:326-363, without the SMPL-vertex branch):
 *   pts [P][3] world -> rgb_feat [P][V][35] = (rgb, 32 features), mask [P][V] (0/1). */
int gpnerf_project_gather(const GpnerfFrame* frame, const float* pts, int64_t n_points, int32_t neg_ray, float* rgb_feat,
                          float* mask, void* stream);

/* NeRFHead.forward on already-gathered features (libs/nerfheads/trainhead.py:159-163, with the
 * sparse volume replaced by its sampled features): P points.
 *   vol_feat [P][128] (level-major), rgb_feat [P][V][35], mask [P][V] (0/1 floats), all device
 *   raw [P][4] = rgb, sigma.   head_blob_ref: the gpnerf_pack_head_ref() image (reference summation order). */
int gpnerf_head_forward(const float* head_blob_ref, const float* vol_feat, const float* rgb_feat, const float* mask,
                        int64_t n_points, float* raw, void* stream);

/* The two halves of the head as the reference's progressive renderer calls them (libs/renders/demo_render.py:295-326):
 * gpnerf_sigma_features = NeRFSigmaHead.test_forward (libs/nerfheads/trainhead.py:61-76) after its volume sampling:
 *   vol_feat [P][128], rgb_feat [P][V][35] -> sigma_feat [P][64] = ELU(Linear(vol_feat)), globalfeat [P][134] =
 *   [sigma_feat, mean over views (35), population variance over views (35)];
 * gpnerf_rgb_head_forward = NeRFRGBHead.forward (:118-145): sigma_feat [P][64], rgb_feat [P][V][35], mask [P][V] ->
 *   raw [P][4] = (rgb_out, sigma_out).  All device; head_blob_ref: the gpnerf_pack_head_ref() image. */
int gpnerf_sigma_features(const float* head_blob_ref, const float* vol_feat, const float* rgb_feat, int64_t n_points,
                          float* sigma_feat, float* globalfeat, void* stream);
int gpnerf_rgb_head_forward(const float* head_blob_ref, const float* sigma_feat, const float* rgb_feat, const float* mask,
                            int64_t n_points, float* raw, void* stream);

/* Renderer.raw2outputs (BaseRender.py:75-107) alone.  raw [N][S][4], z [N][S],
 * nvalid [N][S] = per-sample number of valid views (may be NULL), all device. */
int gpnerf_composite(const float* raw, const float* z_vals, const float* nvalid, int64_t n_rays, int32_t n_samples,
                     int32_t neg, const GpnerfOutputs* out, void* stream);

/* get_rays + get_near_far (libs/datasets/data_utils.py:47-63,96-130) for one target camera, in the precision the dataset
 * runs them in (sample_ray's test branch, :294-300): float64 camera products rounded once to float32 rays, float64 plane hits
 * and on-box tests (`bounds + [-0.01, 0.01]` promotes them, :98), float32 norm_ray, distances rounded to float32.
 * mask_at_box, rays, near and far are bit-exact against the reference's numpy run (tests/golden/rays_*.npz).
 *   Kinv, Rinv: host 3x3 row-major float64 inverses (np.linalg.inv of K, R); cam_o: host [3] float64 camera centre -Rinv @ T;
 *   bounds: host [2][3] float32 world AABB (un-padded).
 *   rays: device [H*W][8]; hit: device [H*W] uint8 (mask_at_box).  Rays are written at their
 *   pixel index; the caller keeps the hit ones in raster order. */
int gpnerf_make_rays(int32_t H, int32_t W, const double* Kinv, const double* Rinv, const double* cam_o,
                     const float* bounds, float* rays, uint8_t* hit, void* stream);

/* SparseConvNet.encode's occupancy volume (libs/nerfheads/networks/SparseConvNet.py:135-139):
 * occ[d][h][w] = sum over the 4 levels of (channel sum of level k, nearest-upsampled to level-1 size).
 * Reads frame->vol / vol_dhw (channels-last); occ: device [D_1][H_1][W_1]. */
int gpnerf_build_occupancy(const GpnerfFrame* frame, float* occ, void* stream);

/* Progressive ray selection of the inference renderer (libs/renders/demo_render.py:166-200): every level-1 voxel with
 * occ > threshold (SparseConvNet.py:140: 0.1) is mapped to a world point (voxel index * 2 * voxel + bounds_min, then
 * @ Rh^T + Th), projected with the target camera (pose 3x4 row-major [R|T], K 3x3), and its 4 neighbouring pixels
 * (truncation toward zero, clamped) are marked in pixel_sel (device [img_h*img_w], cleared here).  world_minmax: device
 * int32[6] = order-preserving integer images of min xyz / max xyz of the world points (decode: i >= 0 ? bits : bits ^ 0x7FFFFFFF).
 * voxel_xyz, bounds_min, Rh, Th, pose, K: host. */
int gpnerf_select_pixels(const float* occ, int32_t D, int32_t H, int32_t W, float threshold, const float* voxel_xyz,
                         const float* bounds_min, const float* Rh, const float* Th, const float* pose, const float* K,
                         int32_t img_h, int32_t img_w, uint8_t* pixel_sel, int32_t* world_minmax, void* stream);
/* The inference renderer's on-device get_rays / near-far (libs/renders/demo_render.py:201-239): pixel_camera = xy1 @ Kinv^T,
 * pixel_world = (pixel_camera - T) @ R, rays_o = (-R^T) @ T, with every length-3 product accumulated as torch's CPU `@` does
 * (fused multiply-adds over k = 0,1,2), the box used as given (no +-0.01), directions not clamped, distances by torch.norm's
 * formula, and under neg_ray the second distance negated.  Kinv: host 3x3 (batch['target_K_inv']); pose: host 3x4 row-major
 * [R|T] (batch['target_pose']); the box: bounds, host [2][3], or -- when world_minmax_dev is not NULL -- what
 * gpnerf_select_pixels left on the device, decoded and z-padded by 0.05 (demo_render.py:168-175) inside the kernel, so the two
 * launches need no host round trip between them.  pixel_sel: optional device [H*W] mask of the pixels to consider
 * (others get hit = 0).  Bit-exact against the reference's CPU run (tests/golden/demo_*.npz). */
int gpnerf_make_rays_demo(int32_t H, int32_t W, const float* Kinv, const float* pose, const float* bounds,
                          const int32_t* world_minmax_dev, int32_t neg_ray, const uint8_t* pixel_sel, float* rays, uint8_t* hit,
                          void* stream);

/* ---- geometry mode of the inference renderer (libs/renders/demo_render.py:249-311,366-376: nerfhead.use_rgbhead False) ----
 *
 * gpnerf_density_lattice: alpha = 1 - exp(-sigma) of the density branch on the lattice axis_x (x) axis_y (x) axis_z (meshgrid 'ij':
 * x slowest), written into cube, device float [X + 2 pad][Y + 2 pad][Z + 2 pad] (X, Y, Z = dims, host int32[3]), with pad zeros on
 * every side (np.pad(cube, 10) at :370).  A point is evaluated iff the occupancy volume frame->occ interpolates to > 0 at its grid
 * coordinates (pts_to_can_pts and the demo's get_grid_coords with its literal / 0.005, :270-283; the cull of
 * GPNERF_FLAG_OCC_CULL); a culled point's alpha is 0.  A kept point's sigma is the reference-order form's (GPNERF_FLAG_REF_ORDER):
 * the four volume levels, the sigma feature layer, Projector.compute of the three views under neg_ray, mean / variance,
 * rgbhead.out_geometry_fc, 0 where no view is valid -- the fused kernel's step without its colour branch.  Every element of the
 * cube is written (the caller does not clear it).  axis_*: device float32 lattice coordinates (frame.lattice_axis() makes them as
 * torch.range does); n_kept: device int64 or NULL, receives the number of kept points.  Needs frame->occ, frame->head_blob_ref,
 * the volumes and the image half of the frame. */
int gpnerf_density_lattice(const GpnerfFrame* frame, const float* axis_x, const float* axis_y, const float* axis_z, const int32_t* dims,
                           int32_t pad, int32_t neg_ray, float* cube, int64_t* n_kept, void* stream);

/* ---- geometry mode of the dense renderer (libs/renders/BaseRender.py:255-272: cfg.head.rgb.use_rgbhead False) ----
 *
 * gpnerf_visual_hull: batch['inside'] -- ZjumocapDataset.prepare_inside_pts (libs/datasets/ZjumocapDataset.py:259-283) with
 * data_utils.project (libs/datasets/data_utils.py:239-250), which the reference runs in numpy on a loader worker for every batch --
 * on the lattice axis_x (x) axis_y (x) axis_z (meshgrid 'ij', x slowest; frame.dataset_lattice_axes() makes the axes of :397-402).
 *   axis_*: device float32; dims: host int32[3], each >= 1, X * Y * Z <= 2^28;
 *   masks: device uint8 [n_views][mask_h][mask_w], the views of self.inside_view in order (get_mask, :68-86: 0, 1 and the erode /
 *     dilate border band's 100); n_views: 1 to 8;
 *   cams: host double [n_views][21] = K 3x3 row-major, then RT 3x4 row-major, T in metres (the reference divides by 1000 at :268);
 *   inside: device uint8 [X][Y][Z], every element written; n_inside: device int64 or NULL, receives the number of non-zero elements
 *     (set by the call: a kernel of the library's own, one integer atomic per wavefront, order-independent).
 * A point's value starts at 1.  For each view in order, only while the value is exactly 1: the float32 point widened to float64,
 * c = p0 RT[:,0] + p1 RT[:,1] + p2 RT[:,2] + RT[:,3], h = c0 K[:,0] + c1 K[:,1] + c2 K[:,2] (float64, multiply then add in that
 * order, unfused), x = h0 / h2, y = h1 / h2, column = clip(int32(rint(x)), 0, mask_w - 1), row likewise (rint: half to even, as
 * np.round); the value becomes masks[view][row][column].  Two quirks of the reference are kept:
 *   - border pixels are sticky: a point that picks up 100 is not 1 any more, no later view tests it, and it stays 100 (the renderer's
 *     .bool() counts it as inside); a point that picks up 0 stays 0.  The output is the value, not a boolean;
 *   - a quotient that is not finite, or whose rounded value does not fit int32, converts to INT32_MIN as numpy's astype does on
 *     x86-64, so the clip gives column / row 0 (tested explicitly, not left to the device's saturating conversion).
 * Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; captures into a HIP graph.  GPNERF_E_ARG for a
 * null pointer (n_inside excepted), n_views outside 1..8, a mask or lattice size < 1, or more than 2^28 points. */
int gpnerf_visual_hull(const float* axis_x, const float* axis_y, const float* axis_z, const int32_t* dims, int32_t n_views,
                       const uint8_t* masks, int32_t mask_h, int32_t mask_w, const double* cams, uint8_t* inside, int64_t* n_inside,
                       void* stream);

/* gpnerf_density_lattice_masked: gpnerf_density_lattice with a caller-given kept set -- the cube of BaseRender.py:262-269
 * (sigma at pts[inside], cube[inside] = 1 - exp(-sigma), np.pad(cube, pad)).  The same kernel (a second instantiation: the same bricks
 * of 4 x 8 points of one x-slice of the padded cube, one lane per point, persistent workgroups), with these differences:
 *   - a point is kept iff inside[i][j][k] != 0 (device uint8 [X][Y][Z]: gpnerf_visual_hull's output or batch['inside']; 100 and 255
 *     keep a point as 1 does);
 *   - grid coordinates are the renderer's (BaseRender.get_grid_coords, the frame's voxel size), the form gpnerf_query_points uses
 *     without GPNERF_FLAG_OCC_CULL; frame->occ is not read;
 *   - a kept point's alpha is, bit for bit, gpnerf_query_points' alpha at the world point (axis_x[i], axis_y[j], axis_z[k]) with
 *     GPNERF_FLAG_DENSITY_ONLY and no cull; every other element of the cube, padding included, is written as 0;
 *   - a 32-point tile with no kept point does no gather and no matrix work; n_kept (device int64 or NULL) is set by the call. */
int gpnerf_density_lattice_masked(const GpnerfFrame* frame, const float* axis_x, const float* axis_y, const float* axis_z,
                                  const int32_t* dims, int32_t pad, int32_t neg_ray, const uint8_t* inside, float* cube,
                                  int64_t* n_kept, void* stream);

/* gpnerf_query_points: the radiance field at n_points caller-given world points -- NeRFHead.forward (trainhead.py:159-163) in the
 * reference-order form (GPNERF_FLAG_REF_ORDER), the arithmetic of the fused kernel's step: grid coordinates (pts_to_can_pts +
 * get_grid_coords), the four volume levels (multiply-then-add trilinear taps), the sigma feature layer, Projector.compute of the three
 * views, mean / variance, the density branch (0 where no view is valid) and the colour branch (sigmoid rgb).  GP-NeRF's colour does
 * not depend on a viewing direction, so a point's rgb is the value the renderer composites there.  Bit for bit: raw at the sample
 * points of a ray equals gpnerf_render_fused's `raw` of the reference-order form; with GPNERF_FLAG_OCC_CULL and the lattice input at
 * the lattice's integer indices, alpha equals gpnerf_density_lattice's cube.  Points keep the caller's order (one lane per point, 32
 * consecutive points per wavefront: spatially coherent lists run faster); the result of a point depends on that point alone.
 *   pts: device float32 [n_points][3], world xyz -- or, with `lattice` (host double[7] = {lo[3], step[3], pad}), index units of a
 *     padded lattice cube (gpnerf_mesh_emit's vertices as they come): each coordinate becomes p = (float)(lo + ((double)v - pad) * step),
 *     in float64, multiply then add, unfused; at v = pad + i that is frame.lattice_axis()'s value i bit for bit when lo is the
 *     float64 value of the float32 axis start and step the float64 voxel size;
 *   raw: device float32 [n_points][4] = r, g, b, sigma (the reference's `raw` layout); alpha: device float32 [n_points] or NULL,
 *     1 - exp(-sigma) as gpnerf_density_lattice computes it;
 *   flags: GPNERF_FLAG_NEG_RAY (Projector(neg_ray)); GPNERF_FLAG_OCC_CULL (grid coordinates with the literal voxel size 0.005, a point
 *     whose occupancy frame->occ interpolates to 0 gets raw = 0 and alpha = 0; a 32-point tile with no kept point does no gather and
 *     no matrix work); GPNERF_FLAG_DENSITY_ONLY (the colour branch is left out, rgb is written as 0).  Other flags are refused.
 * Needs frame->head_blob_ref, the volumes and the image half of the frame (and frame->occ with GPNERF_FLAG_OCC_CULL).  n_points == 0
 * is a no-op. */
#define GPNERF_FLAG_DENSITY_ONLY 512u   /* gpnerf_query_points: sigma (and alpha) only, rgb written as 0 */
int gpnerf_query_points(const GpnerfFrame* frame, const float* pts, int64_t n_points, uint32_t flags, const double* lattice, float* raw,
                        float* alpha, void* stream);

/* Marching cubes over a float32 cube [X][Y][Z] (dims: host int32[3], each >= 2, X * Y * Z <= 2^28; x slowest), iso value iso
 * (the reference's literal 1 / 50 at :372).  Two calls with the same cube, dims, iso and workspace:
 *   gpnerf_mesh_count: counts: device int64[2] <- {n_vertices, n_triangles}; the workspace (gpnerf_mesh_workspace_bytes(dims)
 *     bytes, device) keeps the offsets for
 *   gpnerf_mesh_emit: vertices: device float [n][3], faces: device int32 [m][3]; only the first max_vertices / max_triangles
 *     rows are written (the caller sizes them from the counts).
 * Output, a function of the cube and iso alone (no atomics; independent of launch geometry):
 *   - corner bit set where value < iso; case index = sum of bit(corner c) << c, corners c at offset (c in {1,2,5,6},
 *     c in {2,3,6,7}, c >= 4) from the cell's lowest corner, edges numbered as in the classic tables (0-3 on z = 0, 4-7 on z = 1,
 *     8-11 along z);
 *   - one vertex per crossed lattice edge (an edge whose two ends disagree), ordered by (linear index of the edge's lower end,
 *     axis x < y < z); position = lower end + t along the axis, t = (iso - f0) / (f1 - f0) in float32, lower end f0, upper f1;
 *     in index units of the cube (as mcubes returns them);
 *   - triangles ordered by (linear index of the cell's lowest corner, order in the case table), wound so that the normal
 *     (v1 - v0) x (v2 - v0) points toward lower values;
 *   - the triangle lists (gp-nerf_amd/mesh.py: case_tables) cut every cube face on its own, so that two cells agree on the face they
 *     share: on an ambiguous face the two set corners are cut off separately.  They are NOT the published triangle lists, and
 *     whether PyMCubes' tables and tie rule give the same mesh has not been checked (mcubes is not available to compare with).
 * gpnerf_mesh_workspace_bytes returns 0 for dims it refuses. */
int64_t gpnerf_mesh_workspace_bytes(const int32_t* dims);
int gpnerf_mesh_count(const float* cube, const int32_t* dims, float iso, void* workspace, size_t workspace_bytes, int64_t* counts,
                      void* stream);
int gpnerf_mesh_emit(const float* cube, const int32_t* dims, float iso, const void* workspace, size_t workspace_bytes,
                     int64_t max_vertices, int64_t max_triangles, float* vertices, int32_t* faces, void* stream);

/* Finishing the cube before / the mesh after marching cubes (gpnerf_mesh.hip): floaters, enclosed cavities, vertex normals.  Both
 * entry points: kernel launches only, on the caller's stream; nothing allocated, nothing waited for; a fixed number of launches sized
 * from dims alone (no sweep-until-stable loop, no host read); the call captures into a HIP graph; the result is a function of the
 * inputs alone.  dims as for gpnerf_mesh_count (each >= 2, product <= 2^28, x slowest).
 *
 * gpnerf_cube_clean(cube, dims, iso, flags, min_points, workspace, workspace_bytes, out_cube, labels, stats, stream):
 *   - a point is INSIDE iff !(value < iso): the exact negation of marching cubes' corner bit, so the two never disagree (NaN is inside);
 *   - SOLID COMPONENTS are the inside points under 18-connectivity (6 face + 12 face-diagonal neighbours): the case tables cut every
 *     face on its own and separate the two below-iso corners of an ambiguous face, so the solid is joined across a face diagonal and
 *     not across a body diagonal, and the outside is 6-connected;
 *     labels (device int32 [X][Y][Z], or NULL): for every inside point the linear index of the lowest point of its component, -1 elsewhere;
 *   - GPNERF_CUBE_KEEP: with min_points > 0 every component of at least min_points points is kept; with min_points == 0 only the
 *     largest, a tie going to the component with the lower label; every inside point of a component that is not kept is written as
 *     0.0f.  Without the flag every component is kept (min_points is then ignored; min_points < 0 is refused);
 *   - GPNERF_CUBE_FILL, applied to the cube AFTER the step above (a bubble inside a removed floater has opened and is not filled): the
 *     below-iso points are grouped under 6-connectivity; a component that reaches none of the cube's six boundary faces is a cavity,
 *     and every point of a cavity is written as 1.0f;
 *   - every other element of out_cube is cube's, bit for bit; every element is written.  out_cube must not alias cube (refused);
 *   - stats: device int64[6] = {solid components, inside points, components kept, inside points kept, cavities filled, points filled};
 *   - a cube with no inside point is not an error (out_cube = cube, the stats are zeros); other flag bits are refused;
 *   - workspace: gpnerf_cube_clean_workspace_bytes(dims) bytes on the device (8 per point: a parent word and a count word, the same
 *     two arrays serve both passes; plus one 256-byte line for the selection), contents meaningless between calls.
 *   Zeroing whole solid components and raising whole cavities never touches a value on an edge that still crosses, so every triangle of
 *   the cleaned cube's mesh is a triangle of the unfiltered mesh, positions bit for bit.
 *   Atomics, and why the outcome does not depend on their arrival order (all integer, none float):
 *     - the union-find's parent words only ever decrease (atomicMin of a smaller index of the SAME set), a set's root is the one word
 *       that points at itself, and a union links the larger of two roots below the smaller: whatever the order, the root of a set ends
 *       as its lowest index, which is what the flattening pass (a kernel of its own) writes everywhere;
 *     - sizes, the boundary-face bit and the six stats are integer adds / ors: commutative and associative, no overflow (<= 2^28 points);
 *     - "largest" is one 64-bit atomicMax over (size << 32 | ~label): a total order, so the maximum is the same in any order.
 *
 * gpnerf_mesh_normals(cube, dims, vertices, n_vertices, inv_step, normals, stream): unit normals (device float [n][3]) at any points
 * inside the cube, in index units (device float [n][3]; marching-cubes vertices as they come), from the cube's central differences:
 *   - G(p)[a] = (f(p + e_a) - f(p - e_a)) * 0.5 * inv_step[a] at a lattice point p, the two indices clamped to the cube;
 *     inv_step: host float[3] or NULL = 1, 1, 1 (1 / voxel size gives geometric normals on an anisotropic lattice);
 *   - for a vertex v, per axis: i = clamp(floor(v), 0, dim - 2), t = v - i; g = the trilinear interpolation of G over the cell's eight
 *     corners, lerp along z, then y, then x, each lerp as a + t * (b - a) -- for a marching-cubes vertex the lerp between the two ends
 *     of its edge;
 *   - n = -g / |g|, |g| = sqrt((gx gx + gy gy) + gz gz): toward lower values, the side the triangles' winding faces; n = (0, 0, 0)
 *     exactly when |g| is 0 or not finite; all arithmetic in float32, unfused; n_vertices == 0 is a no-op. */
#define GPNERF_CUBE_KEEP 1u
#define GPNERF_CUBE_FILL 2u
int64_t gpnerf_cube_clean_workspace_bytes(const int32_t* dims);
int gpnerf_cube_clean(const float* cube, const int32_t* dims, float iso, uint32_t flags, int64_t min_points, void* workspace,
                      size_t workspace_bytes, float* out_cube, int32_t* labels, int64_t* stats, void* stream);
int gpnerf_mesh_normals(const float* cube, const int32_t* dims, const float* vertices, int64_t n_vertices, const float* inv_step,
                        float* normals, void* stream);

/* The evaluator's metrics of one rendered view (gpnerf_metrics.hip; libs/evaluators/if_nerf.py:15-63), written into a slot of
 * GPNERF_METRICS_DOUBLES doubles on the device: kernel launches only (four), nothing allocated, nothing waited for, no atomics --
 * the slot is a function of the inputs alone, and the call captures into a HIP graph.
 *   pred, gt: device float [n][3], the mask's pixels in raster order (the renderer's rgb_map and the batch's rgb);
 *   mask: device uint8 [H][W], non-zero = pixel present (torch.bool bytes); workspace: gpnerf_metrics_workspace_bytes(H, W)
 *   bytes on the device, its contents meaningless between calls (one workspace serves one stream's calls in order).
 * The slot:
 *   MSE: the mean over all 3n values of ((double)pred - (double)gt)^2 (PSNR = -10 log10 of it is the host's to take);
 *   SSIM: skimage compare_ssim(multichannel=True)'s defaults on the two images that are zero outside the mask, cropped to the
 *     mask's bounding rectangle: per channel over the (h-6)(w-6) valid 7x7 windows, uniform means of x, y, xx, yy, xy in double,
 *     (co)variances x 49/48, c1 = (0.01 * 2)^2, c2 = (0.03 * 2)^2; the mean over windows, then over channels;
 *   X, Y, W, H: the bounding rectangle of the mask's set pixels (cv2.boundingRect; 0,0,0,0 when empty); POPULATION: their number;
 *   STATUS: 0 ok; 1 the population is not n (MSE and SSIM NaN, neither list is read through the mask); 2 the mask is empty (both NaN);
 *     3 the rectangle is narrower or lower than the window (SSIM NaN, MSE valid).
 * Returns GPNERF_E_ARG (before any device call) for a null pointer, H < 1, W < 1, H * W >= 2^31, n < 0, n > H * W or a workspace
 * that is too small; gpnerf_metrics_workspace_bytes (host arithmetic only) returns 0 for dims the call refuses. */
#define GPNERF_METRICS_MSE 0
#define GPNERF_METRICS_SSIM 1
#define GPNERF_METRICS_X 2
#define GPNERF_METRICS_Y 3
#define GPNERF_METRICS_W 4
#define GPNERF_METRICS_H 5
#define GPNERF_METRICS_POPULATION 6
#define GPNERF_METRICS_STATUS 7
#define GPNERF_METRICS_DOUBLES 8
size_t gpnerf_metrics_workspace_bytes(int32_t H, int32_t W);
int gpnerf_image_metrics(const float* pred, const float* gt, const uint8_t* mask, int32_t H, int32_t W, int64_t n, void* workspace,
                         size_t workspace_bytes, double* out, void* stream);

/* ---- evaluating a mesh against another (gpnerf_meshdist.hip): the exact nearest point of a triangle mesh, area-weighted surface
 * samples, and the reduction of a list of distances.  Point-to-surface distance, Chamfer, normal consistency and F-score are these
 * three.  All entry points: kernel launches only, on the caller's stream; nothing allocated, nothing waited for; a fixed number of
 * launches sized from the arguments alone; every data-dependent length stays on the device; every call captures into a HIP graph
 * and replays with the same bits; the result is a function of the inputs alone (integer atomics only where the arrival order
 * cannot matter -- gpnerf_meshdist.hip says where and why -- and no float atomic).
 * A mesh is vertices: device float [n_vertices][3] and faces: device int32 [n_faces][3], 1 <= n_faces < 2^31.  A face with an index
 * outside [0, n_vertices) or a non-finite vertex is INVALID: skipped, counted, never dereferenced.
 *
 * THE DISTANCE of a point p to a triangle (a, b, c), the one __device__ function every caller uses, in float32, unfused: the
 * vertices are taken relative to p (a - p, ...: one rounding each), dot(u, v) = (ux vx + uy vy) + uz vz, and the closest point is
 * Ericson's (Real-Time Collision Detection 5.1.5), its seven regions tested in his order -- vertex a, vertex b, edge ab, vertex c,
 * edge ca, edge bc, interior -- with an edge's parameter taken as clamp(projection on the edge / |edge|^2, 0, 1) (0 when |edge|^2
 * is 0) and the interior point as a + ab (vb / den) + ac (vc / den), den = (va + vb) + vc.  A triangle whose normal ab x ac is
 * exactly zero (collinear vertices, three equal vertices), or whose den is not positive, is the nearest of its three segments
 * (ab, bc, ca in that order, a strictly smaller squared distance replaces).  distance = sqrt(dot(cp, cp)).  Never NaN for finite input.
 *
 * gpnerf_mesh_grid_build(vertices, n_vertices, faces, n_faces, cell_cap, entry_cap, workspace, workspace_bytes, stream): a uniform
 * cell grid over the bounding box of the valid faces, six launches:
 *   - the box by a min / max reduction; the plan (one thread): extents e in double; cubic cells of edge s = (prod e / cell_cap)^(1/k)
 *     over the k axes of positive extent, n[a] = min(floor(e[a] / s), 1024); an axis with e[a] < s gets ONE cell and the others share
 *     cell_cap again; the product is at most cell_cap; cell size = e / n in float32, 1.0 on an axis of zero extent (a flat mesh is
 *     legal).  cell(x) on an axis = clamp(floor((x - lo) * (1 / size)), 0, n - 1), in float32: monotone in x, defined for every x;
 *   - a face is entered into every cell of cell(min corner) .. cell(max corner) of its own bounding box: count (integer atomic
 *     add), exclusive scan (integers), fill, then every entry is written at run start + the number of smaller faces of its run:
 *     within a cell the entries are in ascending face index whatever order the fill ran in.  That last step costs the sum of the
 *     squared run lengths: choose cell_cap so that runs stay short (the Python wrapper's default does);
 *   - the header, int32 words at the start of the workspace (GPNERF_GRID_HDR_*): STATUS (GPNERF_GRID_OK; GPNERF_GRID_OVERFLOW: the
 *     entries needed exceed entry_cap, NO entry has been written, NEEDED holds the count to retry with), SKIPPED (invalid faces),
 *     VALID, CELLS[3], N_CELLS, CELL_CAP, ENTRY_CAP, NEEDED (int64 in two words, low first), LO[3], SIZE[3], INV[3] (float32 bits).
 *     A mesh with no valid face builds an empty grid (status OK): every distance to it is +inf;
 *   - GPNERF_E_ARG, before any device call: a null pointer, n_vertices < 0, n_faces < 1 or >= 2^31, cell_cap < 1 or > 2^24,
 *     entry_cap < 1 or > 2^30, a workspace under gpnerf_mesh_grid_workspace_bytes(n_faces, cell_cap, entry_cap) (host arithmetic
 *     only; 0 for what the build refuses; 8 bytes per cell + 12 per entry + 33 KiB).
 *
 * gpnerf_mesh_distance(points, n_points, vertices, n_vertices, faces, n_faces, grid_workspace, max_dist, query_normals, dist, face,
 * closest, cosine, stream): for each of the device float [n_points][3] queries
 *   dist (device float [n]): min over the valid faces of THE DISTANCE -- exact, not approximate;  face (device int32 [n]): the face
 *   that attains it, the LOWEST index among faces at bit-equal float32 distance;  closest (device float [n][3] or NULL): p + cp of
 *   that face;  cosine (device float [n] or NULL, given together with query_normals, device float [n][3]): |n_q . n_f|, n_f =
 *   (b - a) x (c - a) / its length in float32, 0 where that length is 0 or not finite or the product is NaN (n_q is used as given).
 *   - max_dist = +inf: exact everywhere.  Finite and positive: exact wherever the result is at most max_dist; elsewhere dist = +inf,
 *     face = -1, closest and cosine NaN.  Zero, negative or NaN is refused.  A mesh without a valid face: +inf / -1 everywhere;
 *   - a query with a non-finite coordinate: dist NaN, face -1, closest and cosine NaN;
 *   - grid_workspace NULL selects the BRUTE-FORCE form: the faces staged through LDS in tiles of 256, every query against every face,
 *     the same distance function, tie rule and max_dist rule: dist and face are bit-equal to the grid form's.  It is the on-device
 *     cross-check and the right form for small meshes.  n_vertices lets it refuse an invalid face by itself;
 *   - grid_workspace: a workspace gpnerf_mesh_grid_build has filled FOR THE SAME vertices, faces and n_faces.  One query per lane;
 *     the search visits the cells in shells r = 0, 1, 2, ... (Chebyshev distance r, in cells, from the query's own cell, clipped
 *     to the grid) and stops behind shell r as soon as best <= B(r) or B(r) >= max_dist, or when every cell has been visited.
 *     A grid whose status is not OK makes every dist NaN (face -1): a half-built grid is never read;
 *   - THE BOUND.  B(r) = (r - 1/16) * w * 0.999, w = the smallest cell size among the axes on which shells 0..r do not yet reach
 *     both ends of the grid.  Proof.  Let T be a face no cell of which lies in shells 0..r.  T's cells are a box of cell indices, so
 *     on some axis a the box lies wholly above q[a] + r or wholly below q[a] - r, q = the query's cell; that axis is one the shells
 *     have not covered from end to end.  Above: cell(Tmin) >= q + r + 1 >= 1, so floor(t(Tmin)) >= q + r + 1 (the clamp at n - 1
 *     only lowers), t(x) = (x - lo) * inv as computed; and floor(t(p)) <= q -- the clamp at 0 only raises, and q = n - 1 by the
 *     upper clamp is impossible here because q + r + 1 <= n - 1.  So t(Tmin) - t(p) > r.  Below is the mirror image: cell(Tmax) <=
 *     q - r - 1 gives t(Tmax) < q - r, and t(p) >= q whether by floor or by the upper clamp.  Both hold for a query OUTSIDE the box:
 *     its coordinate only enters through the one-sided inequality on the side it is clamped to.  The computed t differs from the
 *     real (x - lo) / size by a factor 1 + d, |d| <= 3 * 2^-24, applied to values of magnitude at most n + 1 <= 1025 in these
 *     inequalities, so the real separation exceeds (r - 2^-12) cells: every point of T is farther than (r - 2^-12) * size[a] from p.
 *     The computed distance of such a face errs by at most 2^-20 * (distance + diameter of T), under 0.002 of a cell for any T
 *     inside the grid; the 1/16 and the 0.999 cover both, so no face outside the visited shells can have a computed distance <= B(r):
 *     none can beat or tie the best one, and dist and face equal the brute-force form's bit for bit;
 *   - GPNERF_E_ARG, before any device call: n_points < 0, n_vertices < 0, n_faces < 1, null vertices or faces, a max_dist that is
 *     not > 0, cosine without query_normals or the reverse, and (with n_points > 0) null points, dist or face.  n_points == 0 is a no-op.
 *
 * gpnerf_mesh_sample_surface(vertices, n_vertices, faces, n_faces, n_samples, seed, workspace, workspace_bytes, points, sample_face,
 * sample_normal, stream): n_samples (< 2^31) deterministic area-weighted points on the surface, three launches:
 *   - a face's area is 0.5 |(b - a) x (c - a)| in double from the float32 vertices (0 for an INVALID face, which so receives no sample); the
 *     inclusive prefix sums P are taken in double in one fixed association (four faces in a thread, 256 threads in thread order,
 *     chunks of 1024 faces in chunk order), so P never decreases and is a function of the inputs alone;
 *   - sample i takes the first face f with P[f] > (i + 0.5) / n_samples * total: stratified, every face receives its share to
 *     within one sample, a face of zero area receives none;
 *   - the point is (1 - s) a + s (1 - r2) b + s r2 c, s = sqrt(r1), each coordinate (wa a + wb b) + wc c in float32;
 *     r1 = (h(seed ^ h(2 i)) >> 8) * 2^-24, r2 = (h(seed ^ h(2 i + 1)) >> 8) * 2^-24 in [0, 1), uint32 arithmetic, i's low 32 bits,
 *     h = MurmurHash3's 32-bit finalizer fmix32 (Appleby): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16;
 *   - points: device float [n][3]; sample_face: device int32 [n] or NULL; sample_normal: device float [n][3] or NULL, the face's
 *     (b - a) x (c - a) / its length in float32;
 *   - the workspace (gpnerf_mesh_sample_workspace_bytes(n_faces): 8 bytes per face and a little) starts with an int32 status:
 *     GPNERF_SAMPLE_OK, or GPNERF_SAMPLE_NO_AREA when the total area is zero or not finite: every point is then NaN, every face -1;
 *     the total (double) is at byte 8;
 *   - GPNERF_E_ARG, before any device call: null vertices, faces or workspace, n_vertices < 0, n_faces < 1 or >= 2^31, n_samples < 0
 *     or >= 2^31, a workspace that is too small, null points with n_samples > 0.  n_samples == 0 is a no-op.
 *
 * gpnerf_distance_stats(values, n, thresholds, n_thresholds, out, stream): one slot of GPNERF_DIST_DOUBLES doubles on the device from
 * device float [n] values (distances, or cosines), one launch of one workgroup: every thread adds its values t, t + 256, ... in
 * order in double, then a fixed tree; no atomics.  thresholds: HOST float [n_thresholds], n_thresholds <= GPNERF_DIST_MAX_THRESHOLDS.
 *   FINITE, INF, NAN: the counts of finite, infinite (+inf: beyond max_dist; -inf is counted here too) and NaN values;  MEAN, MEAN_SQ, MAX: of the finite values,
 *   NaN when there is none;  WITHIN + k: the fraction of the non-NaN values that are <= thresholds[k] (an infinite value of either sign is
 *   not within), NaN when there is no non-NaN value or k >= n_thresholds.  n == 0: the counts are 0, everything else NaN.
 *   GPNERF_E_ARG: null out, n < 0, null values with n > 0, n_thresholds outside [0, 4], null thresholds with n_thresholds > 0. */
#define GPNERF_GRID_OK 0
#define GPNERF_GRID_OVERFLOW 1
#define GPNERF_GRID_BUILDING 2
#define GPNERF_GRID_HDR_MAGIC 0
#define GPNERF_GRID_HDR_STATUS 1
#define GPNERF_GRID_HDR_SKIPPED 2
#define GPNERF_GRID_HDR_VALID 3
#define GPNERF_GRID_HDR_CELLS 4
#define GPNERF_GRID_HDR_N_CELLS 7
#define GPNERF_GRID_HDR_CELL_CAP 8
#define GPNERF_GRID_HDR_ENTRY_CAP 9
#define GPNERF_GRID_HDR_NEEDED 10
#define GPNERF_GRID_HDR_LO 12
#define GPNERF_GRID_HDR_SIZE 15
#define GPNERF_GRID_HDR_INV 18
#define GPNERF_GRID_HDR_INTS 64
#define GPNERF_SAMPLE_OK 0
#define GPNERF_SAMPLE_NO_AREA 1
#define GPNERF_DIST_FINITE 0
#define GPNERF_DIST_INF 1
#define GPNERF_DIST_NAN 2
#define GPNERF_DIST_MEAN 3
#define GPNERF_DIST_MEAN_SQ 4
#define GPNERF_DIST_MAX 5
#define GPNERF_DIST_WITHIN 6
#define GPNERF_DIST_MAX_THRESHOLDS 4
#define GPNERF_DIST_DOUBLES 10
size_t gpnerf_mesh_grid_workspace_bytes(int64_t n_faces, int64_t cell_cap, int64_t entry_cap);
int gpnerf_mesh_grid_build(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int64_t cell_cap,
                           int64_t entry_cap, void* workspace, size_t workspace_bytes, void* stream);
int gpnerf_mesh_distance(const float* points, int64_t n_points, const float* vertices, int64_t n_vertices, const int32_t* faces,
                         int64_t n_faces, void* grid_workspace, float max_dist, const float* query_normals, float* dist, int32_t* face,
                         float* closest, float* cosine, void* stream);
size_t gpnerf_mesh_sample_workspace_bytes(int64_t n_faces);
int gpnerf_mesh_sample_surface(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int64_t n_samples,
                               uint32_t seed, void* workspace, size_t workspace_bytes, float* points, int32_t* sample_face,
                               float* sample_normal, void* stream);
int gpnerf_distance_stats(const float* values, int64_t n, const float* thresholds, int32_t n_thresholds, double* out, void* stream);

/* ---- registering a mesh onto a scan (gpnerf_align.hip): the least-squares rigid / similarity fit of given pairs, the transform of
 * a point list, and one trimmed point-to-plane step of ICP (iterative closest point) on the correspondences gpnerf_mesh_distance
 * wrote.  A scan sits millimetres to centimetres off the frame a predicted mesh is extracted in, and at F-score thresholds of 5 mm
 * that offset decides the number; the loop -- transform, nearest point, step, a fixed number of times -- runs without a host read.
 * All entry points: kernel launches only, on the caller's stream; nothing allocated, nothing waited for; a fixed number of launches
 * of a fixed size; every data-dependent decision is taken on the device and leaves a status; no atomics; every call captures into
 * a HIP graph and replays with the same bits.
 *
 * THE SLOT: device double [GPNERF_XFORM_DOUBLES].  M[12]: the row-major 3 x 4 matrix of x -> s R x + t;  SCALE: s;  STATUS:
 * GPNERF_ALIGN_OK, GPNERF_ALIGN_FEW (too few pairs) or GPNERF_ALIGN_SINGULAR;  USED: the pairs that entered the last fit;  SKIPPED:
 * the pairs with a non-finite coordinate, a weight that is not finite and > 0, a face outside [0, n_faces) or INVALID, or a nearest
 * face of zero area;  TRIMMED: the pairs whose distance exceeds max_dist;  WSUM: the sum of the weights used;  RMS: the weighted
 * root-mean-square residual of the used pairs BEFORE the fit (NaN when none was used);  PIVOT[3]: the point c the plane step rotates
 * about.  The counts are whole numbers stored as doubles.  No call ever writes a non-finite number into M or SCALE.
 *
 * THE SUMS.  Everything is double, unfused, from the float32 inputs converted exactly, and every sum has one association: pair i
 * belongs to thread t = i % GPNERF_ALIGN_THREADS of workgroup b = (i / GPNERF_ALIGN_THREADS) % GPNERF_ALIGN_BLOCKS, i.e. thread t of
 * workgroup b adds the terms of the pairs i = (k BLOCKS + b) THREADS + t, k = 0, 1, ..., in ascending k, onto zero; a workgroup's 256
 * partials fold by the halving tree x[t] += x[t + s], s = 128, 64, ..., 1 (gpnerf_distance_stats' tree); the 64 workgroups' rows go
 * to the workspace and the next launch folds them by the same tree from s = 32.  A pair that is skipped or trimmed adds exact zeros
 * and is counted in integers.  dot(u, v) = (ux vx + uy vy) + uz vz;  u x v = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx).
 * The workspace (gpnerf_align_workspace_bytes(), host arithmetic only: 8 GPNERF_ALIGN_WS_DOUBLES) is read as doubles at these
 * indices once a call's launches are through: WS_SUMS1: W, sum w src [3], sum w dst [3];  WS_CENTROIDS: c_src [3], c_dst [3];
 * WS_SUMS2: S[9], sum w |a|^2, sum w |dst - src|^2;  WS_STEP: the plane step's 29 sums;  WS_COUNTS: int64 used, skipped, trimmed;
 * WS_ROWS: the workgroups' rows, [BLOCKS][29];  WS_COUNT_ROWS: int64 [BLOCKS][4].  A call carries nothing over from the workspace.
 *
 * (w, x, y, z) -> R, for a unit quaternion: R = [1 - 2 (yy + zz), 2 (xy - wz), 2 (xz + wy);  2 (xy + wz), 1 - 2 (xx + zz),
 * 2 (yz - wx);  2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy)], every product formed once (xx = x x, wz = w z, ...).
 *
 * gpnerf_rigid_fit(src, dst, weights, n, with_scale, slot, workspace, workspace_bytes, stream): the weighted least-squares
 * x -> s R x + t over the n pairs (src[i], dst[i]) (device float [n][3]; weights: device float [n] or NULL for 1), four launches:
 *   - pass 1: W = sum w, sum w src, sum w dst (term w * coordinate); c_src = sum w src / W, c_dst likewise (0 when no pair is used);
 *   - pass 2, with a = src - c_src, b = dst - c_dst: S[3 r + k] = sum (w a_r) b_k, sum w dot(a, a), and sum w dot(e, e), e = dst - src;
 *   - one thread solves Horn's symmetric 4 x 4 (Closed-form solution of absolute orientation using unit quaternions, 1987):
 *     N00 = (Sxx + Syy) + Szz, N11 = (Sxx - Syy) - Szz, N22 = (Syy - Sxx) - Szz, N33 = (Szz - Sxx) - Syy, N01 = Syz - Szy,
 *     N02 = Szx - Sxz, N03 = Sxy - Syx, N12 = Sxy + Syx, N13 = Szx + Sxz, N23 = Syz + Szy, by cyclic Jacobi: V = I, a fixed 8
 *     sweeps, the pairs (p, q), p < q, in row-major order; a rotation is skipped when A[p][q] == 0; theta = (A[q][q] - A[p][p]) /
 *     (2 A[p][q]), t = sign(theta) / (|theta| + sqrt(theta theta + 1)) (sign(0) = 1), c = 1 / sqrt(t t + 1), s = t c; for k = 0..3
 *     the columns (A[k][p], A[k][q]) <- (c A[k][p] - s A[k][q], s A[k][p] + c A[k][q]), then the rows p, q likewise, then
 *     A[p][q] = A[q][p] = 0, then V's columns like A's;
 *   - the quaternion is V's column at the largest diagonal entry (the lowest index among equal ones), divided by its length
 *     sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3), negated when q0 < 0;  s = 1, or with with_scale (Umeyama's scale for this R)
 *     s = (sum over i, j in row-major order, onto zero, of R[i][j] S[3 j + i]) / sum w |a|^2;
 *     t_i = c_dst_i - s ((R_i0 c_src_0 + R_i1 c_src_1) + R_i2 c_src_2);  M = [s R | t];
 *   - STATUS: fewer than 3 used pairs: _FEW;  sum w |a|^2 not > 0, the four diagonal entries all equal, s not > 0, or anything not
 *     finite: _SINGULAR.  The call writes the slot ABSOLUTELY: M is the identity and SCALE 1 when the status is not _OK.
 *     TRIMMED = 0, PIVOT = c_src, RMS = sqrt(sum w |dst - src|^2 / W): the residual of the pairs as given;
 *   - n == 0 is legal: the sums are empty and the status is _FEW.
 *
 * gpnerf_align_init(points, n, init_matrix12, slot, workspace, workspace_bytes, stream): M = init_matrix12 (HOST double [12],
 * row-major 3 x 4, passed by value; NULL: the identity), SCALE = the length of its first row, STATUS _OK, USED / WSUM = the number of
 * finite points, SKIPPED the others, RMS 0, PIVOT = the unweighted centroid of the finite points (pass 1 above with w = 1; 0 when
 * there is none).  Two launches.
 *
 * gpnerf_transform_points(points, n, slot, vectors, out, stream): out[i] = float32(M p), each coordinate ((m0 x + m1 y) + m2 z) + m3
 * in double, rounded once.  vectors != 0 applies R only: (((m0 / s) x + (m1 / s) y) + (m2 / s) z), s = SCALE, no translation (normals).
 * A point with a non-finite coordinate gives three NaN.  out == points is allowed.  n == 0 is a no-op.
 *
 * gpnerf_align_step(cur, closest, face, dist, n, vertices, n_vertices, faces, n_faces, max_dist, slot, history_row, workspace,
 * workspace_bytes, stream): one point-to-plane Gauss-Newton step.  cur (device float [n][3]) are the source points as the caller
 * transformed them by the slot's M; closest, face, dist are what gpnerf_mesh_distance wrote for cur against the mesh.  Two launches.
 *   - a pair in this order: dist NaN or cur not finite: SKIPPED;  dist > max_dist: TRIMMED;  dist infinite, face outside
 *     [0, n_faces), closest not finite, the face INVALID, or its normal's length not > 0: SKIPPED;  otherwise used;
 *   - per used pair, a, b, c the face's vertices: n_f = (b - a) x (c - a), each component divided by sqrt(dot(n, n));
 *     c' = M PIVOT, each coordinate ((m0 c0 + m1 c1) + m2 c2) + m3;  J = [(p - c') x n_f, n_f];  r = dot(closest - p, n_f);
 *   - the 29 sums: J_u J_v for u <= v in row-major order (21), J_u r (6), r r, and 1 (W);
 *   - one thread solves (sum J J^T) x = sum J r, x = (omega, u), by Cholesky, column by column, every sum a chain of subtractions in
 *     ascending k: d_j = A_jj - L_j0 L_j0 - ...; L_jj = sqrt(d_j); L_ij = (A_ij - L_i0 L_j0 - ...) / L_jj;  y_i = (g_i - L_i0 y_0 -
 *     ...) / L_ii;  x_i = (y_i - L_(i+1)i x_(i+1) - ... - L_5i x_5) / L_ii for i = 5 .. 0.  A pivot d_j that is not > 2^-30 A_jj:
 *     _SINGULAR.  Fewer than 6 used pairs: _FEW (tested first);
 *   - the rotation of the update uses no trigonometry (Cayley), so only + - x / sqrt occur: h = omega / 2, q = (1, h) / sqrt(1 +
 *     ((hx hx + hy hy) + hz hz)) -- 1 / sqrt(..) formed once, then multiplied -- and R from q as above;
 *   - the step p -> R (p - c') + c' + u = R p + ts, ts_i = (c'_i + u_i) - ((R_i0 c'_0 + R_i1 c'_1) + R_i2 c'_2), is composed onto M
 *     on the left: M'_ij = (R_i0 M_0j + R_i1 M_1j) + R_i2 M_2j, j = 0 .. 3, and M'_i3 + ts_i.  SCALE and PIVOT stay;
 *   - a status other than _OK (or a non-finite M', reported as _SINGULAR) leaves M as it was: the step is the identity;
 *   - USED, SKIPPED, TRIMMED, WSUM (= USED), STATUS are written; RMS = sqrt(sum r r / W), the plane residual BEFORE the step;
 *     history_row (device double [4] or NULL) receives RMS, USED, TRIMMED, STATUS.
 *
 * GPNERF_E_ARG, before any device call: a null pointer (weights, init_matrix12 and history_row may be null), n < 0 or >= 2^39, a
 * workspace under gpnerf_align_workspace_bytes(), a max_dist that is not > 0, n_vertices < 0, n_faces < 1 or >= 2^31, a non-finite
 * init_matrix12 or one whose first row is zero. */
#define GPNERF_ALIGN_THREADS 256
#define GPNERF_ALIGN_BLOCKS 64
#define GPNERF_ALIGN_OK 0
#define GPNERF_ALIGN_FEW 1
#define GPNERF_ALIGN_SINGULAR 2
#define GPNERF_XFORM_M 0
#define GPNERF_XFORM_SCALE 12
#define GPNERF_XFORM_STATUS 13
#define GPNERF_XFORM_USED 14
#define GPNERF_XFORM_SKIPPED 15
#define GPNERF_XFORM_TRIMMED 16
#define GPNERF_XFORM_WSUM 17
#define GPNERF_XFORM_RMS 18
#define GPNERF_XFORM_PIVOT 19
#define GPNERF_XFORM_DOUBLES 24
#define GPNERF_ALIGN_WS_SUMS1 0
#define GPNERF_ALIGN_WS_CENTROIDS 8
#define GPNERF_ALIGN_WS_SUMS2 16
#define GPNERF_ALIGN_WS_STEP 32
#define GPNERF_ALIGN_WS_COUNTS 64
#define GPNERF_ALIGN_WS_ROWS 128
#define GPNERF_ALIGN_WS_COUNT_ROWS 1984
#define GPNERF_ALIGN_WS_DOUBLES 2240
size_t gpnerf_align_workspace_bytes(void);
int gpnerf_rigid_fit(const float* src, const float* dst, const float* weights, int64_t n, int32_t with_scale, double* slot, void* workspace,
                     size_t workspace_bytes, void* stream);
int gpnerf_align_init(const float* points, int64_t n, const double* init_matrix12, double* slot, void* workspace, size_t workspace_bytes,
                      void* stream);
int gpnerf_transform_points(const float* points, int64_t n, const double* slot, int32_t vectors, float* out, void* stream);
int gpnerf_align_step(const float* cur, const float* closest, const int32_t* face, const float* dist, int64_t n, const float* vertices,
                      int64_t n_vertices, const int32_t* faces, int64_t n_faces, float max_dist, double* slot, double* history_row,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- drawing a mesh into calibrated cameras (gpnerf_raster.hip): depth and face-id maps, vertex attributes interpolated over them,
 * and the counts that compare the mesh's silhouette with a foreground mask (mask IoU, precision, recall: how a body mesh is judged on
 * data that has cameras and masks but no scan).  All entry points: kernel launches only, on the caller's stream; nothing allocated,
 * nothing waited for; every launch sized from the arguments alone; the one data-dependent length (the large-face list's) stays on
 * the device; every call captures into a HIP graph and replays with the same bits; the result is a function of the inputs alone and
 * of no launch geometry (integer atomics only -- a 64-bit unsigned minimum per covered pixel, integer sums -- and no float atomic).
 * A mesh is vertices: device float [n_vertices][3] and faces: device int32 [n_faces][3], 0 <= n_faces < 2^31 (a pointer may be NULL
 * where its count is 0).  cams: HOST double [n_views][21] = K 3x3 row-major, then RT 3x4 row-major: gpnerf_visual_hull's layout and
 * meaning; n_views: 1 to 8; H, W: 1 to 16384.
 *
 * THE DEFINITION (gpnerf_mesh_rasterize), per view:
 *   - a vertex: the float32 point widened to float64, c = p0 RT[:,0] + p1 RT[:,1] + p2 RT[:,2] + RT[:,3], h = c0 K[:,0] + c1 K[:,1]
 *     + c2 K[:,2] (float64, multiply then add in that order, unfused: gpnerf_visual_hull's projection), z = h2, x = h0 / h2,
 *     y = h1 / h2.  It is USABLE iff x, y and z are finite, z >= z_near and |x| <= 2^20 and |y| <= 2^20.  Its snapped position is
 *     X = int64(rint(256 x)), Y = int64(rint(256 y)) (rint: half to even): 1/256 of a pixel.  The centre of pixel (column i, row j)
 *     is (256 i, 256 j) -- the convention under which the hull's rint(x) picks a pixel;
 *   - a face (a, b, c) is SKIPPED FOR A VERTEX when an index is outside [0, n_vertices) or a vertex is not usable in this view (behind
 *     the near plane, beyond the guard band, not finite); otherwise it is SKIPPED FOR ITS AREA when its doubled area
 *     A = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) (int64, exact) is 0; otherwise it is DRAWN (whether or not it covers a pixel).
 *     There is no backface culling;
 *   - coverage, int64 (no overflow: differences are at most 2^29, products at most 2^58): with P the pixel's centre,
 *     Ea = (Xc - Xb)(Py - Yb) - (Yc - Yb)(Px - Xb), Eb = (Xa - Xc)(Py - Yc) - (Ya - Yc)(Px - Xc), Ec = (Xb - Xa)(Py - Ya) - (Yb - Ya)
 *     (Px - Xa) (Ea + Eb + Ec = A).  The pixel is covered iff Ek sign(A) >= 0 for all three: edges and vertices are inclusive, so two
 *     faces that share an edge both cover a pixel centre on it and the key below decides;
 *   - depth, perspective-correct, float64: wk = double(Ek) / double(A), q = (wa / za + wb / zb) + wc / zc, depth = float(1 / q);
 *   - a pixel keeps the MINIMUM over the drawn faces that cover it of the 64-bit key (bits(depth) << 32) | face index: the nearest
 *     depth, then the smaller face index.
 * Outputs, each optional (NULL):  depth: device float [n_views][H][W], +inf where no face covers;  face_id: device int32
 * [n_views][H][W], -1 there;  stats: device int64 [n_views][4] (GPNERF_RASTER_*): faces DRAWN, SKIPPED_VERTEX, SKIPPED_AREA
 * (their sum is n_faces) and PIXELS covered.
 * Launches: a clear; one lane per (face, view), which walks the face's clipped pixel box -- the pixels whose centres lie in
 * [min X, max X] x [min Y, max Y] and in the image -- unless that box holds more than 256 pixels: such a pair is appended to a
 * list in the workspace (one counter add per wavefront); a launch of fixed grid that reads the list's length on the device and
 * gives each listed pair a wavefront, 64 pixels per step; a resolve that splits the keys (one integer add per wavefront for PIXELS).
 * workspace: gpnerf_mesh_raster_workspace_bytes(n_faces, n_views, H, W) bytes (host arithmetic only; 0 for what the call refuses) =
 * 256 + align256(8 n_views H W) + align256(8 n_faces n_views), align256 rounding up to a multiple of 256: the header, the keys,
 * the list at its worst.  It carries nothing from call to call.
 * GPNERF_E_ARG, before anything is launched: null cams or workspace, null vertices with n_vertices > 0 or faces with n_faces > 0,
 * a count that is negative or >= 2^31, n_views outside 1..8, H or W outside 1..16384, a z_near that is not > 0 and finite, a
 * workspace under the formula.
 *
 * gpnerf_mesh_interpolate(face_id, vertices, n_vertices, faces, n_faces, cams, n_views, H, W, z_near, attrs, C, background, out,
 * stream): attrs: device float [n_vertices][C], C in 1..4; background: HOST float [C]; out: device float [n_views][H][W][C].  At a
 * pixel whose face_id names a face that is drawn in that view (same z_near) and covers the pixel, the face's Ek, wk, zk and q are
 * recomputed as above, uk = (wk / zk) / q, and out = (ua attr_a + ub attr_b) + uc attr_c in float64, rounded to float32; every other
 * pixel (-1, an id outside [0, n_faces), a face that does not cover it) receives background.  One launch.  GPNERF_E_ARG as above,
 * and for null face_id, background or out, null attrs with n_vertices > 0, C outside 1..4.
 *
 * gpnerf_silhouette_stats(face_id, masks, n_views, H, W, out, stream): masks: device uint8 [n_views][H][W] (get_mask: 0, 1 and the
 * border band's 100); out: device int64 [n_views][GPNERF_SILHOUETTE_COUNTS], set by the call.  Per view, over the pixels whose mask
 * is not 100: COVERED (face_id >= 0), GT (mask != 0), BOTH, EITHER; IGNORED: the pixels whose mask is 100 -- the border band is left
 * out, as evaluation on this data does.  IoU = BOTH / EITHER, precision = BOTH / COVERED, recall = BOTH / GT.  Two launches (a zero,
 * a count with one add per wavefront and counter).  GPNERF_E_ARG: a null pointer, n_views outside 1..8, H or W outside 1..16384. */
#define GPNERF_RASTER_DRAWN 0
#define GPNERF_RASTER_SKIPPED_VERTEX 1
#define GPNERF_RASTER_SKIPPED_AREA 2
#define GPNERF_RASTER_PIXELS 3
#define GPNERF_SILHOUETTE_COVERED 0
#define GPNERF_SILHOUETTE_GT 1
#define GPNERF_SILHOUETTE_BOTH 2
#define GPNERF_SILHOUETTE_EITHER 3
#define GPNERF_SILHOUETTE_IGNORED 4
#define GPNERF_SILHOUETTE_COUNTS 5
size_t gpnerf_mesh_raster_workspace_bytes(int64_t n_faces, int32_t n_views, int32_t H, int32_t W);
int gpnerf_mesh_rasterize(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const double* cams,
                          int32_t n_views, int32_t H, int32_t W, double z_near, void* workspace, size_t workspace_bytes, float* depth,
                          int32_t* face_id, int64_t* stats, void* stream);
int gpnerf_mesh_interpolate(const int32_t* face_id, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                            const double* cams, int32_t n_views, int32_t H, int32_t W, double z_near, const float* attrs, int32_t C,
                            const float* background, float* out, void* stream);
int gpnerf_silhouette_stats(const int32_t* face_id, const uint8_t* masks, int32_t n_views, int32_t H, int32_t W, int64_t* out, void* stream);

/* ---- simplifying a mesh by quadric vertex clustering (gpnerf_simplify.hip): the vertices of a cubic cell collapse to one point, the
 * minimiser of the cell's plane quadric, regularised toward the cell's centre and kept inside the cell.  A mesh at the lattice's
 * resolution (one face per lattice step) comes out at the resolution the caller's cell asks for.  Both calls: kernel launches only,
 * on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone; every data-dependent
 * length stays in the workspace; both capture into a HIP graph and replay with the same bits; the result is a function of the
 * inputs alone and of no launch geometry or arrival order (integer atomics for counts and cursors, no float atomic).
 * vertices: device float [n_vertices][3]; faces: device int32 [n_faces][3]; both counts 0 to 2^31 - 1 (a pointer may be NULL where its
 * count is 0); lo: HOST float [3], finite; cell: float, > 0 and finite; cells: HOST int32 [3], each >= 1, product <= 2^26.
 *
 * THE DEFINITION
 *   1. the cell of a vertex v: q_k = floorf((v_k - lo_k) / cell), a float32 subtraction, an IEEE float32 division and a floor, nothing
 *      fused.  The vertex is IN THE GRID iff its coordinates are finite and 0 <= q_k < cells_k on all axes; its cell's linear index
 *      is (q_x cells_y + q_y) cells_z + q_z.
 *   2. a face is VALID iff its three indices are in [0, n_vertices) and its three vertices are in the grid.  Invalid faces are
 *      dropped and counted, never clamped.
 *   3. a cell is OCCUPIED iff a valid face has a vertex in it; the occupied cells, numbered in ascending linear index, are the
 *      CLUSTERS.
 *   4. the quadric of a cluster, float64 on the float32 vertices widened.  Per valid face with corners p0, p1, p2: a = p1 - p0,
 *      b = p2 - p0, n = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x), l = sqrt((n_x n_x + n_y n_y) + n_z n_z); a face with
 *      l == 0 contributes nothing; u = n / l, w = 0.5 l, d = -((u_x p0_x + u_y p0_y) + u_z p0_z), wu = w u, wd = w d; the nine terms
 *      wu_x u_x, wu_x u_y, wu_x u_z, wu_y u_y, wu_y u_z, wu_z u_z (A's upper triangle) and wd u_x, wd u_y, wd u_z (b).  A face
 *      contributes to every DISTINCT cluster among its three, once per cluster.
 *      THE ORDER OF THE SUM: with the cluster's faces sorted by ascending index as entries 0 .. k-1, 64 partial sums start at 0 and
 *      partial j adds entries j, j + 64, ... in order; the sum is ((partial 0 + partial 1) + partial 2) + ... + partial 63.  (For
 *      k <= 64 that is the plain ascending sum.)
 *   5. the position of a cluster in cell (q_x, q_y, q_z), float64: c_k = lo_k + (q_k + 0.5) cell; lambda = (1e-3 ((A_xx + A_yy) + A_zz))
 *      / 3.  If lambda == 0 the position is c.  Otherwise x = c - s where (A + lambda I) s = r, r_i = ((A_ix c_x + A_iy c_y) + A_iz c_z)
 *      + b_i -- the minimiser of the quadric plus lambda |x - c|^2; the matrix is symmetric positive definite with condition number
 *      <= about 3 / 1e-3 -- by Cholesky: l00 = sqrt(m00), l10 = m10 / l00, l20 = m20 / l00, l11 = sqrt(m11 - l10 l10), l21 = (m21 - l20
 *      l10) / l11, l22 = sqrt((m22 - l20 l20) - l21 l21); y0 = r0 / l00, y1 = (r1 - l10 y0) / l11, y2 = ((r2 - l20 y0) - l21 y1) / l22;
 *      s2 = y2 / l22, s1 = (y1 - l21 s2) / l11, s0 = ((y0 - l10 s1) - l20 s2) / l00.  (An x that is not finite -- a quadric that
 *      overflowed -- is replaced by c.)  x is then clamped per axis to the cell's closed box [lo_k + q_k cell, lo_k + (q_k + 1) cell]
 *      (float64); a cluster whose x the clamp changed is counted as CLAMPED; x is rounded to float32 once.
 *   6. every valid face's indices are mapped to cluster ids, corner order kept.  A face with two equal ids is COLLAPSED and dropped.
 *      The others are grouped by their sorted id triple; the parity of a face is the sign of the permutation that sorts its triple;
 *      a group with P faces of parity + and N of parity - has net = P - N.  2 min(P, N) of its faces are counted as CANCELLED
 *      (opposite faces of a sheet that folded shut).  If net == 0 nothing of the group is kept; otherwise exactly one face is: the
 *      lowest original index among those whose parity has the sign of net, and the |net| - 1 others are counted as DUPLICATE.
 *      Output faces are in ascending original index.  (n_faces = out + invalid + collapsed + cancelled + duplicate.)
 *   7. a cluster that no output face references is DROPPED; the others, in ascending cell order, are the output vertices, and the
 *      output faces carry their numbers.  vertex_map[v] = the output vertex of the cluster in v's cell, -1 for a vertex that is not in
 *      the grid or whose cell is no cluster or a dropped one.
 * Every input vertex of a valid face lies within sqrt(3) cell of the position of its cluster (the clamp), up to float32 rounding
 * of the coordinates.
 *
 * gpnerf_mesh_simplify_count does everything that decides and leaves the maps in the workspace; stats: device int64
 * [GPNERF_SIMPLIFY_STATS], set by the call.  The caller reads VERTICES_OUT and FACES_OUT (the one host read), sizes out_vertices
 * float [n][3] and out_faces int32 [m][3], and calls gpnerf_mesh_simplify_emit with the same mesh and workspace; vertex_map: device
 * int32 [n_vertices] or NULL.  Emit reads nothing back: its first launch compares the four sizes it was given with those counted ON
 * THE DEVICE; when they differ, or the workspace holds no finished count, nothing is written and the workspace's 64-bit word
 * GPNERF_SIMPLIFY_HDR_STATUS is GPNERF_SIMPLIFY_MISMATCH (after a good emit: GPNERF_SIMPLIFY_EMITTED).
 * Launches of count: a clear; a lane per vertex (cells); a lane per face (validity, occupancy); a three-launch integer scan of the
 * cells; a lane per face (cluster ids, list lengths); a scan; a lane per face (lists filled by cursor); a lane per (face, corner)
 * that places the face in the cluster's list at the number of smaller faces there -- quadratic in a list's length, but spread over
 * as many lanes as the list has entries --; a wavefront per cluster (quadric in the order above, position); a lane per face that
 * walks the shortest of its three clusters' lists for its group (verdict); two scans (face and vertex numbers); one lane (stats).
 * workspace: gpnerf_mesh_simplify_workspace_bytes(n_vertices, n_faces, cells) bytes (host arithmetic only; 0 for what the calls
 * refuse) = 256 + 5 a(4 nv) + a(8 (nv + 1)) + a(12 nv) + a(4 nf) + 3 a(12 nf) + a(4 C) + a(8 ceil(max(C, nf, nv + 1) / 2048)), with
 * C = cells_x cells_y cells_z and a() rounding up to a multiple of 256.  It carries the maps from count to emit and nothing else.
 * GPNERF_E_ARG, before anything is launched: null lo, cells, workspace or stats; null vertices with n_vertices > 0 or faces with
 * n_faces > 0; a count that is negative or >= 2^31; a cell that is not > 0 and finite; a lo that is not finite; a cells entry < 1 or
 * a product > 2^26; a workspace under the formula (emit: under the formula at C = 1); emit: output sizes that are negative or exceed
 * the input's, a null output whose size is > 0. */
#define GPNERF_SIMPLIFY_VERTICES_OUT 0
#define GPNERF_SIMPLIFY_FACES_OUT 1
#define GPNERF_SIMPLIFY_FACES_INVALID 2
#define GPNERF_SIMPLIFY_FACES_COLLAPSED 3
#define GPNERF_SIMPLIFY_FACES_CANCELLED 4
#define GPNERF_SIMPLIFY_FACES_DUPLICATE 5
#define GPNERF_SIMPLIFY_CLUSTERS_CLAMPED 6
#define GPNERF_SIMPLIFY_CLUSTERS_DROPPED 7
#define GPNERF_SIMPLIFY_STATS 8
#define GPNERF_SIMPLIFY_HDR_STATUS 12
#define GPNERF_SIMPLIFY_COUNTING 1
#define GPNERF_SIMPLIFY_COUNTED 2
#define GPNERF_SIMPLIFY_EMITTED 3
#define GPNERF_SIMPLIFY_MISMATCH 4
size_t gpnerf_mesh_simplify_workspace_bytes(int64_t n_vertices, int64_t n_faces, const int32_t* cells);
int gpnerf_mesh_simplify_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* lo, float cell,
                               const int32_t* cells, void* workspace, size_t workspace_bytes, int64_t* stats, void* stream);
int gpnerf_mesh_simplify_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, void* workspace,
                              size_t workspace_bytes, int64_t n_out_vertices, int64_t n_out_faces, float* out_vertices, int32_t* out_faces,
                              int32_t* vertex_map, void* stream);

/* ---- the adjacency of a mesh, its topology counts and Taubin smoothing (gpnerf_meshtopo.hip): the unique undirected edges of a
 * triangle mesh with their classes, the counts that say whether it is closed and oriented, every vertex's unique neighbours as a
 * CSR, and the lambda | mu filter over that CSR (Taubin 1995: a shrinking pass followed by an inflating one, which smooths the
 * staircase of a marching-cubes surface without shrinking the body the way plain Laplacian smoothing does).  All calls: kernel
 * launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone; every
 * data-dependent length stays in the workspace; both capture into a HIP graph and replay with the same bits; the result is a
 * function of the inputs alone and of no launch geometry, arrival order or order of the faces (integer atomics for counts and
 * cursors, no float atomic; the smoothing has no atomic at all).
 * faces: device int32 [n_faces][3]; n_vertices 0 to 2^31 - 1; n_faces 0 to 715 827 882 (3 n_faces < 2^31: a half-edge's number fits
 * 31 bits); faces may be NULL where n_faces is 0.  Vertex coordinates play no part in the adjacency or the counts.
 *
 * THE DEFINITION
 *   1. a face is USABLE iff its three indices are in [0, n_vertices) and pairwise distinct.  The others are dropped and counted,
 *      never clamped (the rasteriser's and the simplifier's rule).
 *   2. a usable face (a, b, c) contributes the directed HALF-EDGES a -> b, b -> c, c -> a.  An EDGE is a distinct unordered pair
 *      {lo < hi}; its fwd is the number of half-edges lo -> hi, its bwd the number of half-edges hi -> lo, its multiplicity m = fwd + bwd.
 *      m == 1: BOUNDARY.  m == 2 and fwd == bwd == 1: manifold and consistently oriented.  m == 2 otherwise: INCONSISTENT.
 *      m >= 3: NON-MANIFOLD.
 *   3. the stats, int64 [GPNERF_TOPOLOGY_STATS], every one written by the call: FACES_USED, FACES_DROPPED, VERTICES_REFERENCED (by a
 *      usable face), EDGES, BOUNDARY_EDGES, NONMANIFOLD_EDGES, INCONSISTENT_EDGES, EULER = VERTICES_REFERENCED - EDGES + FACES_USED,
 *      BOUNDARY_VERTICES (the vertices on a boundary or non-manifold edge), MAX_VALENCE (the largest number of neighbours).  The mesh
 *      is CLOSED iff it has no boundary and no non-manifold edge, ORIENTED iff no inconsistent and no non-manifold edge, WATERTIGHT iff
 *      both.  Connected components, and with them the genus, are counted by gpnerf_mesh_components (below) on a finished adjacency.
 *   4. the ADJACENCY, a CSR inside the workspace at gpnerf_mesh_adjacency_layout's byte offsets: start int64 [n_vertices + 1] (start[0]
 *      = 0), neighbours int32 with a capacity of 6 n_faces of which start[n_vertices] = 2 EDGES entries are in use -- vertex v's
 *      neighbours, the other ends of its edges, each once, in ASCENDING index at start[v] .. start[v + 1] --, and vertex_flags uint8
 *      [n_vertices]: GPNERF_VERTEX_REFERENCED | GPNERF_VERTEX_BOUNDARY (on a boundary or non-manifold edge).
 *   5. SMOOTHING.  One ITERATION is two Jacobi passes, the first with factor t = lam, the second with t = mu.  A pass reads the old
 *      positions and writes new ones for every vertex i that has k >= 1 neighbours and is not pinned: per coordinate, in float64 on
 *      the float32 positions widened, nothing fused: s = 0.0; for the neighbours j in ascending index s = s + x_j; then
 *      x_i' = float32(x_i + t (s / k - x_i)).  Every other vertex is copied as it is.  PINNED, with GPNERF_SMOOTH_PIN_BOUNDARY: the
 *      vertices flagged GPNERF_VERTEX_BOUNDARY.  A vertex no usable face references has no neighbour and never moves.  Values that
 *      are not finite propagate as IEEE has them.  iterations == 0 is a copy.  The order of the sum is the neighbours' index, not
 *      the faces' order: shuffling a mesh's faces changes no bit of the adjacency or of the smoothed vertices.
 *
 * gpnerf_mesh_adjacency fills the workspace and sets stats (device).  Launches: a clear; a lane per face (usable?, one integer atomic
 * per half-edge on the list length of its lower vertex); a three-launch integer scan (64-bit starts); a lane per face (lists filled
 * by cursor with the keys (hi, 3 face + corner, direction)); a lane per half-edge that walks the list of its lower vertex and counts
 * the half-edges of its edge by direction and those of them with a smaller key -- the one with none is the edge's head: it classifies
 * the edge and adds 1 to both ends' degrees; no sorted copy of the lists is needed, since nothing but these counts is read from
 * them, and the faces used and the edges are counted by the two scans (a third of the half-edges, half the neighbour entries) --; a scan; a lane per half-edge (heads fill both ends' neighbour lists by cursor); a lane per half-edge (heads
 * place both entries at the number of smaller entries in their list: the ascending order); a lane per vertex (counts over the
 * vertices); one lane (stats).  The two walks are quadratic in a vertex's number of half-edges / neighbours but spread over as many
 * lanes: nothing at a valence of 6, and the hub of a fan of 3 000 triangles costs 6 000 x 6 000 + 3 001 x 3 001 short steps.
 * gpnerf_mesh_smooth(vertices float [n_vertices][3] -> out_vertices float [n_vertices][3], which may be the same array) runs 2
 * iterations launches of a lane per vertex on a workspace gpnerf_mesh_adjacency filled for a mesh of n_vertices vertices; when the
 * workspace holds no finished adjacency of that many vertices the launches write nothing.  Between the passes the positions live in
 * the workspace as two float4 arrays (a neighbour is one 16-byte load); the first pass reads `vertices`, the last writes
 * `out_vertices`.  lam, mu: double.  flags: 0 or GPNERF_SMOOTH_PIN_BOUNDARY.
 * workspace: gpnerf_mesh_adjacency_workspace_bytes(n_vertices, n_faces) bytes (host arithmetic only, from the worst-case capacities
 * -- 3 n_faces half-edges, 6 n_faces neighbour entries, two float4 position arrays --, so that no host read is needed anywhere; 0
 * for what the calls refuse) = 256 + 2 a(8 (nv + 1)) + a(nv) + 2 a(16 nv) + 2 a(4 (nv + 1)) + 2 a(4 nv) + a(8 ceil((nv + 1) / 2048))
 * + 2 a(24 nf) + a(3 nf), with a() rounding up to a multiple of 256.  gpnerf_mesh_adjacency_layout (host only): offsets[
 * GPNERF_ADJACENCY_START / _NEIGHBOURS / _VERTEX_FLAGS] = the byte offsets of the three arrays of 4. inside the workspace, each a
 * multiple of 256.
 * GPNERF_E_ARG, before anything is launched: a null workspace, stats or offsets; null faces with n_faces > 0; null vertices or
 * out_vertices with n_vertices > 0; a count that is negative or beyond the limits above; a workspace under the formula (smooth:
 * under the formula at n_faces = 0); smooth: lam outside (0, 1], mu outside [-1, 0], either not finite, iterations outside
 * [0, 10 000], an unknown flag. */
#define GPNERF_TOPOLOGY_FACES_USED 0
#define GPNERF_TOPOLOGY_FACES_DROPPED 1
#define GPNERF_TOPOLOGY_VERTICES_REFERENCED 2
#define GPNERF_TOPOLOGY_EDGES 3
#define GPNERF_TOPOLOGY_BOUNDARY_EDGES 4
#define GPNERF_TOPOLOGY_NONMANIFOLD_EDGES 5
#define GPNERF_TOPOLOGY_INCONSISTENT_EDGES 6
#define GPNERF_TOPOLOGY_EULER 7
#define GPNERF_TOPOLOGY_BOUNDARY_VERTICES 8
#define GPNERF_TOPOLOGY_MAX_VALENCE 9
#define GPNERF_TOPOLOGY_STATS 10
#define GPNERF_VERTEX_REFERENCED 1
#define GPNERF_VERTEX_BOUNDARY 2
#define GPNERF_ADJACENCY_START 0
#define GPNERF_ADJACENCY_NEIGHBOURS 1
#define GPNERF_ADJACENCY_VERTEX_FLAGS 2
#define GPNERF_SMOOTH_PIN_BOUNDARY 1u
size_t gpnerf_mesh_adjacency_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int gpnerf_mesh_adjacency_layout(int64_t n_vertices, int64_t n_faces, int64_t* offsets);
int gpnerf_mesh_adjacency(const int32_t* faces, int64_t n_faces, int64_t n_vertices, void* workspace, size_t workspace_bytes, int64_t* stats,
                          void* stream);
int gpnerf_mesh_smooth(const float* vertices, int64_t n_vertices, void* workspace, size_t workspace_bytes, int32_t iterations, double lam,
                       double mu, uint32_t flags, float* out_vertices, void* stream);

/* ---- the connected components of a mesh (gpnerf_meshcomp.hip): a label per vertex and face, a table with every component's counts
 * and Euler characteristic, and the mesh of the components the caller keeps (all, the largest, those of at least min_faces faces).
 * It is what tells how many pieces a mesh has and drops the floaters of a mesh that has no alpha cube to clean (a loaded scan, a
 * simplified mesh, the hull mesh).  Both calls: kernel launches only, on the caller's stream; nothing allocated, nothing waited for;
 * every launch sized from the arguments alone; every data-dependent length stays in the workspace; both capture into a HIP graph
 * and replay with the same bits.  The labels come from a lock-free min-label union-find over the faces (gpnerf_unionfind.h, the
 * scheme of the cube's components): a FIXED number of launches, no device-wide barrier, no cooperative launch, and no lane ever
 * waits for a value another lane has yet to write.
 * faces: device int32 [n_faces][3]; n_vertices 0 to 2^31 - 1; n_faces 0 to 715 827 882 (the adjacency's limits); faces may be NULL
 * where n_faces is 0.  adjacency_workspace: the workspace gpnerf_mesh_adjacency filled for THIS mesh (same faces, n_vertices and
 * n_faces), of adjacency_bytes >= gpnerf_mesh_adjacency_workspace_bytes(n_vertices, n_faces) bytes; it is read, never written.
 *
 * THE DEFINITION
 *   1. USABLE faces are the adjacency's: indices in [0, n_vertices), pairwise distinct.  G is the graph whose nodes are the vertices a
 *      usable face references and whose edges are the unique undirected edges of the usable faces: exactly what the adjacency's CSR
 *      stores.
 *   2. a COMPONENT is a connected component of G: VERTEX connectivity.  Two sheets that touch in a single vertex are one component.
 *      (This differs from trimesh.split's default, which joins faces across shared EDGES only and would give two.)
 *   3. label[v] = the smallest vertex index of v's component, -1 for a vertex no usable face references.  The components are numbered
 *      0 .. C - 1 in ascending label.  vertex_component int32 [n_vertices]: the number of v's component, -1 for an unreferenced vertex.
 *      face_component int32 [n_faces]: the number of the component of the face's vertices, -1 for a face that is not usable.
 *   4. the TABLE, int64 [C][GPNERF_COMPONENT_COLS] inside the workspace with a capacity of floor(n_vertices / 3) rows (a component has
 *      at least three vertices) of which only the first C are defined: LABEL, VERTICES, EDGES (half the sum of the CSR degrees of the
 *      component's vertices), FACES (usable faces), EULER = VERTICES - EDGES + FACES, BOUNDARY_VERTICES (the component's vertices flagged
 *      GPNERF_VERTEX_BOUNDARY: on a boundary or non-manifold edge).
 *   5. the stats, int64 [GPNERF_COMPONENT_STATS], every one written by the call: COMPONENTS = C; CLOSED_COMPONENTS (rows with
 *      BOUNDARY_VERTICES == 0); LARGEST, the number of the component with the most FACES, a tie going to the lower number (the maximum
 *      of the packed word FACES << 32 | ~number: the total order of the cube's largest component), -1 when C == 0; LARGEST_FACES,
 *      LARGEST_VERTICES, LARGEST_EULER (that row's, 0 when C == 0); KEPT_COMPONENTS, KEPT_VERTICES, KEPT_FACES (the selection's).
 *   6. SELECTION.  keep = GPNERF_COMPONENTS_KEEP_ALL: every component is kept; _KEEP_LARGEST: the component LARGEST; _KEEP_MIN_FACES:
 *      those with FACES >= min_faces (min_faces >= 1; it is ignored by the other two).  The kept vertices are the REFERENCED vertices of
 *      the kept components in ascending original index, the kept faces the USABLE faces of the kept components in ascending original
 *      index, their indices renumbered.  An unreferenced vertex and an unusable face are always dropped: KEEP_ALL is "remove the
 *      unreferenced vertices and the unusable faces".  The kept coordinates are copied bit for bit.
 *   7. every output is a function of n_vertices and the SET of faces: labels, table and stats do not depend on the order of the faces,
 *      on the launch geometry or on the arrival order; face_component and the emitted faces follow the given face order.  Only integer
 *      atomics are used: the union-find's atomicMin (the final roots are the sets' minima whatever the order of the links), integer
 *      sums, one packed 64-bit maximum; no float is computed.
 * The genus of a component is (2 - EULER) / 2 when the component is closed, the mesh has no inconsistent and no non-manifold edge
 * (gpnerf_mesh_adjacency's stats) and EULER is even; a pinched vertex (all of its edges manifold, but its link more than one cycle)
 * is NOT detected and makes that figure wrong.
 *
 * gpnerf_mesh_components fills the workspace and sets stats (device).  Launches: an initialisation (parent[v] = the smaller of v and
 * its smallest neighbour, the first entry of its CSR run; the table zeroed, the header); a lane per face (usable: unite (a, b) and
 * (b, c) -- two read-only walks first, the linking union with its path compression only when they end at different roots); a lane per vertex behind that kernel boundary (flatten: plain
 * loads, label = the root or -1, roots marked); a three-launch integer scan of the root marks (numbers, C); a lane per vertex
 * (vertex_component; VERTICES, the degree and the boundary flag added to the component's row) and a lane per face (face_component;
 * FACES) -- a wavefront whose active lanes share a component adds once per wavefront, the wavefronts of a workgroup that agree once
 * per workgroup, so that a mesh of ONE component issues one add per counter and workgroup instead of one per lane on one address;
 * a mixed wavefront adds once per distinct component among its lanes --; a lane per table row (EDGES halved, EULER, the closed count, the packed
 * maximum, the rows of at least min_faces); a lane per vertex and face (keep marks); two scans (the new numbers); one lane (stats).
 * Every launch first compares the adjacency's header words with n_vertices and n_faces: on a workspace that holds no finished
 * adjacency of this mesh nothing is written to stats, labels, numbers or table, and the workspace's 64-bit word
 * GPNERF_COMPONENTS_HDR_STATUS says GPNERF_COMPONENTS_NO_ADJACENCY (only that header and scan scratch inside the workspace are touched).
 * gpnerf_mesh_components_emit writes the kept mesh: out_vertices float [n_out_vertices][3], out_faces int32 [n_out_faces][3],
 * vertex_map int32 [n_vertices] (old -> new, -1 for a dropped vertex) or NULL, kept_vertices int32 [n_out_vertices] (new -> old: one
 * index_select carries any per-vertex attribute over) or NULL.  The caller reads KEPT_VERTICES and KEPT_FACES (the one host read) and
 * sizes the outputs; emit reads nothing back: its first launch compares n_vertices, n_faces and the two output sizes with those
 * counted ON THE DEVICE; when they differ, or the workspace holds no finished count, nothing is written and the status word is
 * GPNERF_COMPONENTS_MISMATCH (after a good emit: GPNERF_COMPONENTS_EMITTED).  Then a lane per vertex and a lane per face.
 * workspace: gpnerf_mesh_components_workspace_bytes(n_vertices, n_faces) bytes (host arithmetic only, from the worst-case capacities,
 * so that no host read is needed; 0 for what the calls refuse) = 256 + 4 a(4 nv) + 2 a(4 nf) + a(48 floor(nv / 3)) +
 * a(8 ceil(max(nv, nf, 1) / 2048)), with a() rounding up to a multiple of 256: the header; label, vertex_component, the root numbers and
 * the new vertex numbers; face_component and the new face numbers; the table; the scans' block sums.  gpnerf_mesh_components_layout
 * (host only): offsets[GPNERF_COMPONENTS_LABEL / _VERTEX_COMPONENT / _FACE_COMPONENT / _TABLE] = the byte offsets of the four arrays
 * inside the workspace, each a multiple of 256, so that a caller hands out views and copies nothing.
 * GPNERF_E_ARG, before anything is launched: a null workspace, adjacency_workspace, stats or offsets; null faces with n_faces > 0;
 * emit: null vertices with n_vertices > 0, a null out_vertices / out_faces whose size is > 0; a count that is negative or beyond the
 * limits above; an unknown keep; min_faces < 1 with KEEP_MIN_FACES; a workspace or an adjacency workspace under its formula; emit:
 * output sizes that are negative or exceed the input's. */
#define GPNERF_COMPONENT_LABEL 0
#define GPNERF_COMPONENT_VERTICES 1
#define GPNERF_COMPONENT_EDGES 2
#define GPNERF_COMPONENT_FACES 3
#define GPNERF_COMPONENT_EULER 4
#define GPNERF_COMPONENT_BOUNDARY_VERTICES 5
#define GPNERF_COMPONENT_COLS 6
#define GPNERF_COMPONENTS_COMPONENTS 0
#define GPNERF_COMPONENTS_CLOSED_COMPONENTS 1
#define GPNERF_COMPONENTS_LARGEST 2
#define GPNERF_COMPONENTS_LARGEST_FACES 3
#define GPNERF_COMPONENTS_LARGEST_VERTICES 4
#define GPNERF_COMPONENTS_LARGEST_EULER 5
#define GPNERF_COMPONENTS_KEPT_COMPONENTS 6
#define GPNERF_COMPONENTS_KEPT_VERTICES 7
#define GPNERF_COMPONENTS_KEPT_FACES 8
#define GPNERF_COMPONENT_STATS 9
#define GPNERF_COMPONENTS_KEEP_ALL 0
#define GPNERF_COMPONENTS_KEEP_LARGEST 1
#define GPNERF_COMPONENTS_KEEP_MIN_FACES 2
#define GPNERF_COMPONENTS_LABEL 0
#define GPNERF_COMPONENTS_VERTEX_COMPONENT 1
#define GPNERF_COMPONENTS_FACE_COMPONENT 2
#define GPNERF_COMPONENTS_TABLE 3
#define GPNERF_COMPONENTS_HDR_STATUS 3
#define GPNERF_COMPONENTS_COUNTING 1
#define GPNERF_COMPONENTS_COUNTED 2
#define GPNERF_COMPONENTS_EMITTED 3
#define GPNERF_COMPONENTS_MISMATCH 4
#define GPNERF_COMPONENTS_NO_ADJACENCY 5
size_t gpnerf_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int gpnerf_mesh_components_layout(int64_t n_vertices, int64_t n_faces, int64_t* offsets);
int gpnerf_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, const void* adjacency_workspace, size_t adjacency_bytes,
                           int32_t keep, int64_t min_faces, void* workspace, size_t workspace_bytes, int64_t* stats, void* stream);
int gpnerf_mesh_components_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, void* workspace,
                                size_t workspace_bytes, int64_t n_out_vertices, int64_t n_out_faces, float* out_vertices, int32_t* out_faces,
                                int32_t* vertex_map, int32_t* kept_vertices, void* stream);

/* ---- repairing a loaded mesh (gpnerf_meshrepair.hip): weld, de-duplicate, orient outward.  Every other mesh tool here assumes what
 * marching cubes makes: vertices shared between faces, no face twice, one winding, normals out.  A scanner's triangle soup, a merged
 * OBJ with repeated faces and mixed windings, an inside-out export break that silently (every edge a boundary edge, one component
 * per triangle, a wrong sign of the distance field).  This call makes such a mesh fit for them.  Both calls: kernel launches only, on
 * the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone; every data-dependent length
 * stays in the workspace; a fixed number of launches for given flags; no device-wide barrier, no cooperative launch, and no lane ever
 * waits for a value another lane has yet to write; both capture into a HIP graph and replay with the same bits.
 * vertices: device float [n_vertices][3]; faces: device int32 [n_faces][3]; n_vertices 0 to 2^30; n_faces 0 to 715 827 882 (the
 * adjacency's limit); either may be NULL where its count is 0.  tol: finite and >= 0.  flags: GPNERF_REPAIR_WELD | _DROP_DUPLICATES |
 * _ORIENT | _OUTWARD (OUTWARD needs ORIENT).
 *
 * THE DEFINITION
 *   1. KEYS.  A vertex is UNKEYABLE when a coordinate is not finite, or tol > 0 and some |double(x) / tol| >= 2^62.  Otherwise its key
 *      is, with tol == 0, the three float32 bit patterns with -0.0 taken as +0.0; with tol > 0, the three int64 floor(double(x) / tol).
 *      The tol > 0 form is CELL CLUSTERING on the grid of step tol through the origin, not distance welding: two vertices closer than
 *      tol on opposite sides of a cell wall do not weld; two vertices of one cell, up to sqrt(3) tol apart, do.
 *   2. WELD.  With GPNERF_REPAIR_WELD rep[i] = the smallest index among the keyable vertices with i's key; without it rep[i] = i.  An
 *      unkeyable vertex has no representative.  A representative keeps its own coordinates bit for bit; nothing is averaged.
 *   3. FACE FATES, one per ORIGINAL face (a, b, c), the first that applies: GPNERF_REPAIR_INVALID (an index outside [0, n_vertices));
 *      _UNKEYABLE (a corner is an unkeyable vertex); _COLLAPSED (two of rep[a], rep[b], rep[c] are equal); _DUPLICATE (with
 *      GPNERF_REPAIR_DROP_DUPLICATES: some face of lower original index that reached this step has the same unordered set {rep[a],
 *      rep[b], rep[c]}, whatever its winding); _KEPT or _KEPT_FLIPPED for all others: the LIVE faces, in ascending original index.
 *   4. OUTPUT VERTICES: the representatives a live face references, in ascending original index.  kept_vertices maps new -> old;
 *      vertex_map[i] = the new index of rep[i], -1 when rep[i] is not kept or i is unkeyable (a welded vertex maps to where it went);
 *      face_map maps new -> old.  An output face is (new[rep[a]], new[rep[b]], new[rep[c]]), or (a, c, b) of that when it is flipped.
 *   5. PATCHES (with GPNERF_REPAIR_ORIENT).  An edge is an unordered pair of output vertices, m the number of live half-edges on it.
 *      Two live faces are JOINED when they share an edge with m == 2; a PATCH is a connected component of the live faces under JOINED.
 *      This is EDGE connectivity -- non-manifold edges (m >= 3) and boundary edges (m == 1) join nothing -- and NOT the vertex
 *      connectivity of gpnerf_mesh_components: two sheets that touch in a vertex, or along an edge three faces share, are patches of
 *      their own, each wound by itself.  The patch's ROOT is its lowest original face index; face_patch[new face] = the root's
 *      original index (without ORIENT: the face's own original index).  A joined pair has PARITY 1 when its two half-edges run the
 *      same way, 0 otherwise.  A patch is ORIENTABLE when flips s(f) in {0, 1} exist with s(f) xor s(g) = the parity of every joined
 *      pair; with s(root) = 0 they are unique.  An unorientable patch (a Moebius strip) has s = 0 everywhere and is counted.  A patch
 *      is CLOSED when every edge of every one of its faces has m == 2 -- counting, on a non-manifold edge, the half-edges of THE PATCH'S
 *      OWN faces: two solids that share an edge (m == 4, two half-edges of each) are two closed patches, each with a volume of its own;
 *      three sheets on one edge are three open ones.
 *   6. WHICH WAY (orientable patches only).  With GPNERF_REPAIR_OUTWARD, for CLOSED patches: the exact integer signed volume of the
 *      patch after its flips on a quantised grid.  Per axis a: lo_a, hi_a = the float32 minimum and maximum over the output vertices;
 *      c_a = (double(lo_a) + double(hi_a)) / 2; ext = max_a (double(hi_a) - double(lo_a)); q_a(x) = int64(rint((double(x) - c_a) *
 *      (1048574.0 / ext))), every q = 0 where ext == 0; unfused double arithmetic, round half to even.  |q| <= 524 287, so a face's
 *      det(q(A), q(B), q(C)) is below 2^60 in magnitude; per patch hi = det >> 30 (arithmetic) and lo = det & (2^30 - 1) are summed in
 *      two int64 words, both below 2^60 at the face limit: the order of the adds cannot matter.  A negative total inverts every s of
 *      the patch (counted as inverted); a zero total is counted as undecided and treated like an open patch.  Open patches, undecided
 *      patches and every patch without OUTWARD: when more than half of the patch's faces have s = 1 every s is inverted, so that the
 *      minority flips; on an exact half the root keeps its winding.  A flipped face (a, b, c) is written as (a, c, b).
 *      CAVITIES: each closed patch is turned to enclose positive volume BY ITSELF, so the wall of an enclosed cavity ends up facing
 *      its own outside, like the outer wall.  Voxelising with the parity rule is unchanged by that; the nonzero rule fills the
 *      cavity.  A caller who wants neither leaves OUTWARD off (the majority rule then leaves a consistently wound wall alone).
 *   7. the stats, int64 [GPNERF_REPAIR_STATS], every one written by the call: VERTICES_OUT, FACES_OUT; VERTICES_WELDED (keyable and
 *      not their own representative), VERTICES_UNKEYABLE, VERTICES_UNREFERENCED (representatives no live face references);
 *      FACES_INVALID, FACES_UNKEYABLE, FACES_COLLAPSED, FACES_DUPLICATE; FACES_FLIPPED; EDGES_NONMANIFOLD (edges with m >= 3);
 *      PATCHES, PATCHES_CLOSED, PATCHES_UNORIENTABLE, PATCHES_INVERTED, PATCHES_UNDECIDED (the last six are 0 without ORIENT).
 *      n_faces = FACES_OUT + FACES_INVALID + FACES_UNKEYABLE + FACES_COLLAPSED + FACES_DUPLICATE and n_vertices = VERTICES_OUT +
 *      VERTICES_WELDED + VERTICES_UNKEYABLE + VERTICES_UNREFERENCED.
 *   8. every output is a function of the inputs: it does not depend on the launch geometry, the arrival order or the hash function.
 *      The vertex outputs and all stats do not depend on the order of the faces either, with two exceptions where a tie rule names a
 *      face index: which duplicate survives, and the exact half of step 6.  Integer atomics only; no float is summed.
 *
 * gpnerf_mesh_repair fills the workspace and sets stats (device).  Three open-addressing hash tables live in the workspace, each of
 * the smallest power of two >= 2 n slots and at least 64 (n = n_vertices, n_faces, 3 n_faces), cleared by a kernel of the library:
 * vertices (an int32 slot holds a vertex index, its key read through the index), faces (an int32 slot holds a face index, its key
 * the sorted triple of representatives) and edges (a 64-bit slot holds the packed (lo, hi) itself; beside it an incidence count
 * and the first two incidences (face, direction)); a fourth, of the edge table's capacity, counts the half-edges per (non-manifold
 * edge, patch) for step 5's CLOSED.  Insert: probe; CAS the own index into an empty slot; atomicMin it into a slot
 * whose occupant has an equal key; go on otherwise.  A slot never empties and never changes its key, so a key ends in one slot whatever
 * the races and that slot ends holding the key's minimum; a second kernel, behind the kernel boundary, looks the answers up.  Launches:
 * the clear; a lane per vertex (insert, with WELD); a lane per vertex (rep); a lane per face (the first three fates; insert, with
 * DROP_DUPLICATES); a lane per face (DUPLICATE, the live marks, the half-edges into the edge table); with ORIENT: a lane per vertex
 * (the bounding box, with OUTWARD), a lane per face (a lock-free union-find over the faces whose word packs (parent << 1) | parity:
 * find accumulates the parity along the walk, a link hangs the higher root under the lower by CAS with parity p_a xor p_b xor p_edge
 * and retries from find when the CAS fails, a pair found under one root is CHECKED instead and a mismatch marks the face), a lane per
 * face (flatten; faces, flipped faces, the open and mismatch marks and the determinant's two words into the root's row, reduced
 * per wavefront and per workgroup where the lanes agree on the root), two lanes per face with a non-manifold edge (its patch's own
 * half-edges on it, counted and looked up), a lane per root (the decision), a lane per face (the fate);
 * two three-launch scans (the new numbers); one lane (stats).
 * gpnerf_mesh_repair_emit writes out_vertices float [n_out_vertices][3], out_faces int32 [n_out_faces][3] and the maps, each of which
 * may be NULL: vertex_map int32 [n_vertices], kept_vertices int32 [n_out_vertices], face_map int32 [n_out_faces], face_fate uint8
 * [n_faces], face_patch int32 [n_out_faces].  The caller reads VERTICES_OUT and FACES_OUT (the one host read) and sizes the outputs;
 * emit's first launch compares n_vertices, n_faces and the two output sizes with those counted ON THE DEVICE: when they differ
 * nothing is written and the workspace's 64-bit word GPNERF_REPAIR_HDR_STATUS says GPNERF_REPAIR_MISMATCH; on a workspace with no
 * finished count nothing is written and it says GPNERF_REPAIR_NO_COUNT; after a good emit GPNERF_REPAIR_EMITTED.
 * workspace: gpnerf_mesh_repair_workspace_bytes(n_vertices, n_faces) bytes (host arithmetic only, from the worst-case capacities; 0
 * for what the calls refuse) = 256 + 2 a(4 nv) + a(4 Cv) + 2 a(nf) + 3 a(4 nf) + a(4 Cf) + 2 a(8 Ce) + 3 a(4 Ce) + a(56 nf) +
 * a(8 ceil(max(nv, nf, 1) / 2048)), with a() rounding up to a multiple of 256 and Cv, Cf, Ce the three capacities: the header; rep and
 * the new vertex numbers; the vertex table; the fates and the open / mismatch marks; the new face numbers, the union-find's words
 * and the flattened (root, parity); the face table; the edge table's keys and incidences (8 bytes each), its counts and the per-patch table's slots and counts (4 each); the patches' rows (seven
 * int64 per face: a root is a face); the scans' block sums.
 * GPNERF_E_ARG, before anything is launched: a null workspace or stats; null vertices / faces / out_vertices / out_faces whose count
 * is > 0; a count that is negative or beyond the limits above; a tol that is negative or not finite; unknown flag bits; OUTWARD
 * without ORIENT; a workspace under its formula; emit: output sizes that are negative or exceed the input's. */
#define GPNERF_REPAIR_WELD 1u
#define GPNERF_REPAIR_DROP_DUPLICATES 2u
#define GPNERF_REPAIR_ORIENT 4u
#define GPNERF_REPAIR_OUTWARD 8u
#define GPNERF_REPAIR_KEPT 0
#define GPNERF_REPAIR_KEPT_FLIPPED 1
#define GPNERF_REPAIR_INVALID 2
#define GPNERF_REPAIR_UNKEYABLE 3
#define GPNERF_REPAIR_COLLAPSED 4
#define GPNERF_REPAIR_DUPLICATE 5
#define GPNERF_REPAIR_VERTICES_OUT 0
#define GPNERF_REPAIR_FACES_OUT 1
#define GPNERF_REPAIR_VERTICES_WELDED 2
#define GPNERF_REPAIR_VERTICES_UNKEYABLE 3
#define GPNERF_REPAIR_VERTICES_UNREFERENCED 4
#define GPNERF_REPAIR_FACES_INVALID 5
#define GPNERF_REPAIR_FACES_UNKEYABLE 6
#define GPNERF_REPAIR_FACES_COLLAPSED 7
#define GPNERF_REPAIR_FACES_DUPLICATE 8
#define GPNERF_REPAIR_FACES_FLIPPED 9
#define GPNERF_REPAIR_EDGES_NONMANIFOLD 10
#define GPNERF_REPAIR_PATCHES 11
#define GPNERF_REPAIR_PATCHES_CLOSED 12
#define GPNERF_REPAIR_PATCHES_UNORIENTABLE 13
#define GPNERF_REPAIR_PATCHES_INVERTED 14
#define GPNERF_REPAIR_PATCHES_UNDECIDED 15
#define GPNERF_REPAIR_STATS 16
#define GPNERF_REPAIR_HDR_STATUS 3
#define GPNERF_REPAIR_COUNTING 1
#define GPNERF_REPAIR_COUNTED 2
#define GPNERF_REPAIR_EMITTED 3
#define GPNERF_REPAIR_MISMATCH 4
#define GPNERF_REPAIR_NO_COUNT 5
size_t gpnerf_mesh_repair_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int gpnerf_mesh_repair(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, double tol, uint32_t flags,
                       void* workspace, size_t workspace_bytes, int64_t* stats, void* stream);
int gpnerf_mesh_repair_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, void* workspace,
                            size_t workspace_bytes, float* out_vertices, int64_t n_out_vertices, int32_t* out_faces, int64_t n_out_faces,
                            int32_t* vertex_map, int32_t* kept_vertices, int32_t* face_map, uint8_t* face_fate, int32_t* face_patch,
                            void* stream);

/* ---- voxelising a mesh (gpnerf_voxelize.hip): the SOLID occupancy of a triangle mesh on a lattice, packed one bit per lattice point,
 * the counts that give its volume, and the small operations on packed cubes that go with it (from a density cube, back to a float
 * cube, the popcounts of two cubes for a volumetric IoU, containment of points).  It is the one direction mesh -> lattice beside
 * marching cubes' lattice -> mesh: voxelising the marching-cubes mesh of a cube on that cube's own lattice gives back cube > iso.
 * All entry points: kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the
 * arguments alone; the one data-dependent length (the large-face list's) stays on the device; every call captures into a HIP graph
 * and replays with the same bits; the result is a function of the inputs alone and of no launch geometry, of no order of the faces
 * and, under rule PARITY, of no orientation of the faces (integer atomics only -- XOR of a bit, add of +-1, integer sums).
 * A mesh is vertices: device float [n_vertices][3] and faces: device int32 [n_faces][3], both counts 0 to 2^31 - 1 (a pointer may be
 * NULL where its count is 0).  lattice: HOST double [6] = lo[3], step[3], finite, step > 0.  dims: HOST int32 [3] = (nx, ny, nz), each
 * >= 1, product <= 2^28 (marching cubes' limit).  Lattice point (i, j, k) sits at lo + (i, j, k) * step: these are lattice POINTS --
 * what gpnerf_density_lattice samples and marching cubes reads --, not cell centres.  The ray axis is z: the cube's contiguous axis
 * and a standing body's long axis, so it has the fewest columns.  A COLUMN is the nz points of one (i, j).
 *
 * THE DEFINITION (gpnerf_mesh_voxelize)
 *   - a vertex: the float32 point widened to float64, u_a = (p_a - lo_a) / step_a per axis (subtract, then divide).  It is USABLE iff
 *     u_x, u_y, u_z are finite and |u_x| <= 2^16 and |u_y| <= 2^16.  X = int64(rint(4096 u_x)), Y = int64(rint(4096 u_y)) (rint: half to
 *     even): 1/4096 of a lattice step; Z = u_z stays float64.  Column (i, j) is the point (4096 i, 4096 j).  Differences are at most
 *     2^29 and products at most 2^58: the rasteriser's bounds;
 *   - a face (a, b, c) is SKIPPED FOR A VERTEX when an index is outside [0, n_vertices) or a vertex is not usable; otherwise it is
 *     SKIPPED FOR ITS AREA when A = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) (int64, exact) is 0 -- a face that is vertical in projection
 *     bounds no column, so it contributes nothing, correctly --; otherwise it is USED;
 *   - ownership, int64, HALF-OPEN: with P the column, Ea, Eb, Ec exactly as gpnerf_mesh_rasterize writes them -- the edge vectors
 *     (dx, dy) are c - b, a - c, b - a, and Ek = dx (Py - Qy) - dy (Px - Qx) with Q the edge's first vertex (b, c, a) --, s = sign(A): the
 *     face OWNS the column iff for each of the three edges either s Ek > 0, or Ek == 0 and (s dy < 0, or s dy == 0 and s dx > 0).  That
 *     is: a column on an edge belongs to the face it enters when nudged by (eps, eps^2).  Two faces that share an edge never both own
 *     a column on it unless they fold over each other there (where 0 or 2 is right), and of a fan of faces around a vertex exactly
 *     one owns a column on the vertex;
 *   - the crossing of an owned column, float64, unfused: wk = double(Ek) / double(A), z = (wa Za + wb Zb) + wc Zc,
 *     kc = clamp(ceil(z), 0, nz): the number of the column's lattice points strictly below the crossing.  A column through a vertex
 *     has two Ek == 0 and receives that vertex's Z exactly.  Nothing is clipped in z: faces above or below the lattice count;
 *   - the occupancy of point (i, j, k).  Rule GPNERF_VOXEL_PARITY: the number of crossings of its column with kc > k is odd.  Rule
 *     GPNERF_VOXEL_NONZERO: the sum of s over those crossings is not 0 -- overlapping closed parts unite instead of cancelling, which
 *     scans made of separate parts need.  A column is OPEN when the same test over ALL its crossings (kc >= 0) is true: the surface
 *     leaks there (a closed surface crosses every column an even number of times, with signs that cancel).
 * Outputs.  bits: device uint32 [nx][ny][nzw], nzw = ceil(nz / 32): point k is bit (k & 31) of word (k >> 5); bits at or above nz are
 * zero.  stats: device int64 [GPNERF_VOXEL_STATS], set by the call: faces USED, SKIPPED_VERTEX, SKIPPED_AREA (their sum is n_faces),
 * CROSSINGS (the (face, column) pairs owned), OPEN_COLUMNS, OCCUPIED (points; times the product of the steps it is the volume).
 * Launches: a clear; one lane per face, which walks the face's clipped column box -- the columns in [min X, max X] x [min Y, max Y]
 * and in the lattice -- unless that box holds more than 256 columns (the rasteriser's threshold for its pixels, taken over untuned):
 * such a face is appended to a list in the workspace (one counter add per wavefront); a launch of fixed grid that reads the list's
 * length on the device and gives each listed face a wavefront, 64 columns per step; a resolve.  A crossing does ONE no-return atomic
 * at place kc of its column's TOGGLE ROW of nz + 1 places in the workspace -- PARITY: the XOR of one bit, NONZERO: an int32 add of s --
 * and never flips the points below it (nz / 32 atomics per crossing); the resolve takes the suffix XOR / suffix sum down each column,
 * writes bits and counts OCCUPIED and OPEN_COLUMNS with one add per wavefront.
 * workspace: gpnerf_mesh_voxelize_workspace_bytes(n_faces, dims, rule) bytes (host arithmetic only; 0 for what the call refuses) =
 * 256 + align256(4 nx ny T) + align256(4 n_faces), T = nz / 32 + 1 (integer division) under PARITY and nz + 1 under NONZERO, align256
 * rounding up to a multiple of 256: the header, the toggle rows, the list at its worst.  It carries nothing from call to call.
 * GPNERF_E_ARG, before anything is launched: null lattice, dims, workspace, bits or stats; null vertices with n_vertices > 0 or faces
 * with n_faces > 0; a count that is negative or >= 2^31; a dims entry < 1 or a product > 2^28; a lattice entry that is not finite or
 * a step that is not > 0; a rule that is neither; a workspace under the formula.
 *
 * Packed cubes (bits as above; dims as above; GPNERF_E_ARG for a null pointer or bad dims):
 * gpnerf_voxel_from_cube(cube, dims, iso, bits, stream): cube: device float [nx][ny][nz]; bits = cube > iso (false for a NaN), packed.
 * gpnerf_voxel_unpack(bits, dims, cube, stream): cube: device float [nx][ny][nz], 1.0f where the bit is set and 0.0f elsewhere, so that
 * a voxelised scan goes through gpnerf_mesh_count / _emit at iso 0.5 and through gpnerf_cube_clean.
 * gpnerf_voxel_stats(a, b, dims, out, stream): out: device int64 [GPNERF_VOXEL_COUNTS], set by the call: the set bits of A, of B, of
 * BOTH, of EITHER, by popcount over the words (two launches: a zero, a count with one add per wavefront and counter).  b may be NULL:
 * B = BOTH = 0 and EITHER = A.  IoU = BOTH / EITHER, precision = BOTH / A, recall = BOTH / B.
 * gpnerf_voxel_contains(bits, dims, lattice, points, n, out, stream): points: device float [n][3]; out: device uint8 [n].  A point maps
 * to the index rint((p_a - lo_a) / step_a) per axis (float64, half to even): the nearest lattice point; out is 1 iff the three indices
 * are inside dims and that point's bit is set; a coordinate that is not finite or an index outside gives 0.  0 <= n < 2^31; points
 * and out may be NULL where n is 0 (nothing is launched). */
#define GPNERF_VOXEL_PARITY 0
#define GPNERF_VOXEL_NONZERO 1
#define GPNERF_VOXEL_USED 0
#define GPNERF_VOXEL_SKIPPED_VERTEX 1
#define GPNERF_VOXEL_SKIPPED_AREA 2
#define GPNERF_VOXEL_CROSSINGS 3
#define GPNERF_VOXEL_OPEN_COLUMNS 4
#define GPNERF_VOXEL_OCCUPIED 5
#define GPNERF_VOXEL_STATS 6
#define GPNERF_VOXEL_A 0
#define GPNERF_VOXEL_B 1
#define GPNERF_VOXEL_BOTH 2
#define GPNERF_VOXEL_EITHER 3
#define GPNERF_VOXEL_COUNTS 4
size_t gpnerf_mesh_voxelize_workspace_bytes(int64_t n_faces, const int32_t* dims, int32_t rule);
int gpnerf_mesh_voxelize(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const double* lattice,
                         const int32_t* dims, int32_t rule, void* workspace, size_t workspace_bytes, uint32_t* bits, int64_t* stats,
                         void* stream);
int gpnerf_voxel_from_cube(const float* cube, const int32_t* dims, float iso, uint32_t* bits, void* stream);
int gpnerf_voxel_unpack(const uint32_t* bits, const int32_t* dims, float* cube, void* stream);
int gpnerf_voxel_stats(const uint32_t* a, const uint32_t* b, const int32_t* dims, int64_t* out, void* stream);
int gpnerf_voxel_contains(const uint32_t* bits, const int32_t* dims, const double* lattice, const float* points, int64_t n, uint8_t* out,
                          void* stream);

/* ---- the truncated signed distance field of a mesh on a lattice (gpnerf_sdf.hip): at every lattice point the distance to the mesh
 * where it is within a band, the band elsewhere, negative where the voxeliser's bit is set; and the trilinear value of such a field at
 * points.  Marching cubes at an iso value of it is the surface at that metric offset from the mesh.  Mesh, lattice and dims as the
 * voxeliser takes them (above).  Both entry points: kernel launches only, on the caller's stream; nothing allocated, nothing waited
 * for; every launch sized from the arguments alone; the one data-dependent length (the large-face list's) stays on the device; every
 * call captures into a HIP graph and replays with the same bytes; the result is a function of the inputs alone and of no launch
 * geometry, of no arrival order and -- the face ids aside -- of no order of the faces (integer atomics only: a 64-bit minimum, integer sums).
 *
 * THE DEFINITION (gpnerf_mesh_sdf)
 *   - lattice point (i, j, k) is the float32 point P with P_a = float32(lo_a + double(i_a) * step_a): product and sum in float64, one
 *     rounding;
 *   - a face is SKIPPED FOR A VERTEX under the voxeliser's rule extended to all three axes: an index outside [0, n_vertices), or a
 *     vertex with a u_a = (p_a - lo_a) / step_a (float64, subtract then divide) that is not finite or has |u_a| > 2^16, on ANY axis;
 *   - the BOX of every other face, per axis, float64: mn, mx = the least and largest of its three float32 coordinates,
 *     i0 = ceil(((mn - band) - lo_a) / step_a) - 1, i1 = floor(((mx + band) - lo_a) / step_a) + 1, clipped to [0, n_a - 1]: the face's
 *     extent widened by the band and ONE lattice step.  The face is SKIPPED FOR ITS BOX when the clipped range is empty on an axis
 *     (it lies farther than the band from the lattice), otherwise it is USED;
 *   - m(P) = the minimum over the USED faces of THE DISTANCE of gpnerf_mesh_distance (float32, unfused: the closest point of the
 *     triangle relative to P, then sqrt of its dot product with itself); the face of P = the LOWEST index among the faces whose
 *     distance has the same bits;
 *   - if m(P) <= band: |sdf| = m(P) and face_id = that face; otherwise |sdf| = band and face_id = -1 (`<=`: the rule
 *     gpnerf_mesh_distance has for max_dist);
 *   - the sign: sdf = -|sdf| where the point's bit in `bits` is set -- negative inside, the usual convention; a point on the surface is
 *     +0 or -0 by its bit.  The sign is the lattice point's own occupancy: it is known everywhere, beyond the band too, and it is
 *     not an exact sign at distances under a step.  bits NULL: no value is negative (the unsigned field).
 * For a mesh whose faces are all USED or SKIPPED FOR THEIR BOX, |sdf| and face_id at every lattice point EQUAL, bit for bit, what
 * gpnerf_mesh_distance(P, max_dist = band) writes for the query P, in either of its forms, with +inf read as band (and its face -1):
 * both translation units compile the same distance function (csrc/gpnerf_tridist.h).
 * WHY NO POINT OUTSIDE A FACE'S BOX CAN HAVE A COMPUTED DISTANCE <= band.  Let P be a lattice point whose index on some axis a lies
 * outside [i0, i1], say below: i <= ceil(x) - 2 < x - 1 with x = ((mn - band) - lo_a) / step_a, so lo_a + i step_a < mn - band - step_a
 * (the float64 roundings of x move it by 2^-52 of its size).  The exact point therefore lies more than band + step_a from the face
 * along axis a alone, and so does its true distance D.  Against that margin of one step stand (1) the rounding of P to float32, at
 * most 2^-24 |P_a|: under 1/16 step wherever float32 resolves the lattice at all, |P_a| <= 2^20 step_a -- a lattice beyond that has
 * neighbouring points that round to one float32 and no use for a distance to them --, and (2) the distance function's error, at most
 * 2^-20 (D + diameter of the face) (gpnerf_mesh_distance, above): a usable face spans at most 2^17 steps per axis, a diameter under
 * 2^18 steps of an isotropic lattice, so under 1/4 step + 2^-20 D.  A computed distance <= band would need D (1 - 2^-20) <= band +
 * step_a (1/4 + 1/16 sqrt(3)) < band + 0.36 step_a, and D > band + step_a: it cannot, with more than half a step of room (band <=
 * 1024 steps: 2^-20 D is under 0.001 step).  On a lattice whose steps differ the same holds while the face's diameter is under
 * 2^19 of the SMALLEST steps, which every face of a mesh the lattice resolves is.  So the minimum over a point's boxes is the minimum
 * over all USED faces wherever that is <= band, and elsewhere both are above it.
 * Outputs.  sdf: device float [nx][ny][nz].  face_id: device int32 of the same shape, or NULL.  stats: device int64
 * [GPNERF_SDF_STATS], set by the call: faces USED, SKIPPED_VERTEX, SKIPPED_BOX (their sum is n_faces); LARGE: the used faces that went
 * through the list; IN_BAND: the lattice points with m <= band; INSIDE: the points whose bit is set; VISITED: the (face, point)
 * pairs evaluated, i.e. the sum of the used faces' box sizes; PAIRS: those of them with a distance <= band, which bounds the atomics
 * issued from above (the number issued depends on arrival order and is not counted).
 * band: float, finite, > 0, at most 1024 x the smallest step.  bits: gpnerf_mesh_voxelize's packed occupancy for the same lattice and
 * dims (device uint32 [nx][ny][ceil(nz / 32)]), or NULL.
 * Launches: a clear (a kernel of the library's own: every key to all ones); one lane per face, which tests the face, computes its box
 * and walks the box's points -- unless the box holds more than 64 points (one step of a wavefront): such a face is appended to a list
 * in the workspace (one counter add per wavefront); a launch of fixed grid that reads the list's length on the device and gives each
 * listed face a wavefront, 64 points of the box per step, z fastest; a resolve, one lane per lattice point, which turns key and bit
 * into sdf and face_id and counts IN_BAND and INSIDE with one add per wavefront and counter.  At a point a lane evaluates the
 * distance d, and where d <= band the point's uint64 key takes the unsigned MINIMUM with (bits(d) << 32) | face -- one atomic, no
 * return value; d >= +0, so its bits order as the floats do, and the low word makes the lower face win a tie.  A relaxed read of
 * the key first skips the atomic where the key is already as low: keys only fall, so a stale read can only let a needless atomic
 * through.  With a band of a few steps every face of a body-sized mesh (faces of about a step) is in the wavefront tier.
 * workspace: gpnerf_mesh_sdf_workspace_bytes(n_faces, dims) bytes (host arithmetic only; 0 for what the call refuses) =
 * 256 + align256(8 nx ny nz) + align256(4 n_faces): the header, a key per lattice point, the list at its worst.  It carries nothing
 * from call to call.
 * GPNERF_E_ARG, before anything is launched: everything gpnerf_mesh_voxelize refuses of the arguments they share (null lattice, dims,
 * workspace or stats; null vertices with n_vertices > 0 or faces with n_faces > 0; a count that is negative or >= 2^31; a dims entry
 * < 1 or a product > 2^28; a lattice entry that is not finite or a step that is not > 0; a workspace under the formula); a null sdf;
 * a band that is NaN, infinite, <= 0 or above 1024 x the smallest step.
 *
 * gpnerf_sdf_sample(sdf, dims, lattice, points, n, out, stream): the trilinear value of a field (device float [nx][ny][nz], dims each
 * >= 2) at device float [n][3] points, into device float [n]; one lane per point.  Per axis, float64: u_a = (p_a - lo_a) / step_a
 * (subtract, then divide); the result is NaN when a coordinate is not finite or a u_a lies outside [0, n_a - 1]; the cell is
 * c_a = floor(u_a), lowered to n_a - 2 where u_a == n_a - 1, and t_a = u_a - c_a.  The eight corners, widened to float64, are
 * interpolated along z, then y, then x, each time as a + t (b - a), unfused; the result is rounded once to float32.  At a lattice
 * point every t is 0 (or 1 in the last cell, where a + (b - a) gives b back for any two floats with |a| < 2^29 |b| or b = 0) and the
 * stored value comes back (a stored -0 as +0).  Values beyond the band are the band's: the interpolant saturates there.
 * 0 <= n < 2^31; points and out may be NULL where n is 0 (nothing is launched).  GPNERF_E_ARG: a null sdf, dims or lattice, a dims
 * entry < 2 or a product > 2^28, a lattice entry that is not finite or a step that is not > 0, an n outside its range. */
#define GPNERF_SDF_USED 0
#define GPNERF_SDF_SKIPPED_VERTEX 1
#define GPNERF_SDF_SKIPPED_BOX 2
#define GPNERF_SDF_LARGE 3
#define GPNERF_SDF_IN_BAND 4
#define GPNERF_SDF_INSIDE 5
#define GPNERF_SDF_VISITED 6
#define GPNERF_SDF_PAIRS 7
#define GPNERF_SDF_STATS 8
#define GPNERF_SDF_LARGE_POINTS 64
#define GPNERF_SDF_MAX_BAND_STEPS 1024
size_t gpnerf_mesh_sdf_workspace_bytes(int64_t n_faces, const int32_t* dims);
int gpnerf_mesh_sdf(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const double* lattice,
                    const int32_t* dims, float band, const uint32_t* bits, void* workspace, size_t workspace_bytes, float* sdf,
                    int32_t* face_id, int64_t* stats, void* stream);
int gpnerf_sdf_sample(const float* sdf, const int32_t* dims, const double* lattice, const float* points, int64_t n, float* out,
                      void* stream);

/* ---- casting rays against a mesh (gpnerf_raycast.hip): what does a ray hit?  The nearest face of a triangle mesh along each ray of a
 * list in the renderer's row layout, so that a mesh's depth compares element for element with a rendered depth; whether anything lies
 * between two points (visibility, shadow and occlusion rays); and the rays through the pixel centres of calibrated cameras.  Both entry
 * points: kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments
 * alone; NO atomics; every call captures into a HIP graph and replays with the same bytes; the result is a function of the inputs alone.
 * A mesh is gpnerf_mesh_distance's: vertices device float [n_vertices][3], faces device int32 [n_faces][3], 1 <= n_faces < 2^31; a face
 * with an index outside [0, n_vertices) or a non-finite vertex is INVALID: skipped, never dereferenced.  A ray is a row of eight floats
 * (o[3], d[3], tmin, tmax): the points o + t d, tmin <= t <= tmax, d as given and NOT normalised, so t is the renderer's z_vals / depth.
 *
 * THE INTERSECTION of a ray with a triangle (a, b, c), the one __device__ function both forms use (gpnerf_raytri.h), in float32,
 * unfused: the watertight test of Woop, Benthin and Wald (JCGT 2013).
 *   - axes: kz = the axis of the largest |d|, the lowest index on a tie; kx = (kz + 1) % 3, ky = (kx + 1) % 3, the two swapped when
 *     d[kz] < 0;  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz];
 *   - the vertices relative to the origin, A = a - o (one rounding per component), sheared: Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy
 *     A[kz], Az = Sz A[kz]; the same for B and C;
 *   - edge functions f(P, Q) = Px Qy - Py Qx:  U = f(C, B), V = f(A, C), W = f(B, A).  If any of the three is exactly 0, all three are
 *     recomputed in float64 from the float32 sheared coordinates (both products are exact there, so the signs are exact); the miss
 *     test below reads the float64 values, which are then rounded to float32;
 *   - MISS when one of U, V, W is < 0 and another is > 0 (no back-face culling);  det = (U + V) + W, MISS when det == 0;
 *   - T = (U Az + V Bz) + W Cz, t = T / det;  HIT iff tmin <= t <= tmax (both ends inclusive; a NaN fails);  the barycentric weights
 *     of b and c are V / det and W / det.
 * It is watertight: f is exactly antisymmetric in float32 and a nonzero float32 sign is the exact sign, so a face is accepted iff the
 * ray lies in the CLOSED exact triangle of its float32 sheared vertices, and two faces that share an edge or a vertex share those
 * vertices bit for bit: no gap between them (gpnerf_raytri.h carries the argument).
 *
 * gpnerf_mesh_raycast(rays, n_rays, vertices, n_vertices, faces, n_faces, grid_workspace, mode, t, face, bary, stream): for each of the
 * device float [n_rays][8] rays, with mode GPNERF_RAYCAST_NEAREST:
 *   t (device float [n]): the minimum over the valid faces that THE INTERSECTION accepts of its t;  face (device int32 [n]): the face
 *   that attains it, the LOWEST index among faces at bit-equal t;  bary (device float [n][2] or NULL): that face's weights of b and c.
 *   - no face accepted: t = +inf, face = -1, bary NaN;
 *   - a ray with a non-finite component of o or d, d = 0, a NaN bound, or tmin > tmax: t = NaN, face = -1, bary NaN (infinite bounds
 *     are legal);
 *   - GPNERF_RAYCAST_ANY stops at the first accepted face: t = 0 for such a ray (occluded) and +inf for a free one, face = the face
 *     it stopped at (-1 when free), bary NaN.  WHETHER a ray is occluded is the same in both forms and equals "NEAREST hits"; WHICH
 *     face is reported depends on the order the form meets the faces in (the brute-force form: the lowest index; the grid form: the
 *     first in walk order) -- a function of the inputs all the same;
 *   - grid_workspace NULL selects the BRUTE-FORCE form: the faces staged through LDS in tiles of 256, every ray against every face.
 *     One launch.  It is the on-device cross-check and the right form for small meshes;
 *   - grid_workspace: a workspace gpnerf_mesh_grid_build has filled FOR THE SAME vertices, faces and n_faces.  Two launches: the
 *     faces' largest cell span per axis (below; written into the first three words of each row of the workspace's partial boxes,
 *     which the build has finished with -- the only thing the call writes there), then THE WALK, one ray per lane.  A grid whose
 *     status is not OK makes every t NaN (face -1, bary NaN) and is neither read nor written;
 *   - t, face and bary of the two forms are EQUAL BIT FOR BIT (NEAREST);
 *   - GPNERF_E_ARG, before any device call: n_rays < 0, n_vertices < 0, n_faces < 1 or >= 2^31, null vertices or faces, a mode that is
 *     neither of the two, and (with n_rays > 0) null rays, t or face.  n_rays == 0 is a no-op.
 *
 * THE WALK.  Notation: u = 2^-24; lo, size, n: the grid's; r_k(x) = (x - lo_k) / size_k, a coordinate in cells; rho_k(s) = r_k(o_k + s
 * d_k), the ray in cells; z = kz, the axis of the largest |d|, x and y the other two; zeta(s) = rho_z(s) where d_z > 0 and n_z - rho_z(s)
 * where d_z < 0, which grows with s; slab j is the layer of cells with index j on z counted in the direction of travel.  R = max over
 * the axes of |o_k - lo_k| + 1.001 n_k size_k, which bounds |v_k - o_k| for every valid vertex v (all lie in the grid's box).
 * pad_k = 2^-20 R / size_k + 2^-11, in cells.  span_z = the largest cell(max corner) - cell(min corner) on z over the valid faces.
 * The walk's own arithmetic is float64 (its rounding, 2^-52 of quantities no larger than R / size_k, vanishes in the pads).
 *   1. [b0, b1] = the parameters at which the ray is inside the box padded by pad_k on every axis (an axis with d_k = 0 either
 *      contains the ray or ends the walk).  Empty: no hit.
 *   2. The slabs j = first .. last in order, first = max(floor(zeta(b0) - pad_z), floor(zeta(tmin) - pad_z) - span_z, 0), last =
 *      min(floor(zeta(b1) + pad_z), n_z - 1).
 *   3. Before slab j: stop if j > floor(zeta(min(tmax, best)) + pad_z) + span_z, best = the smallest t accepted so far (+inf: none).
 *   4. In slab j, of cell index c on z: sa, sb = the parameters at which rho_z = c - 2^-11 and c + 1 + 2^-11; on x the cells
 *      clamp(floor(min(rho_x(sa), rho_x(sb)) - pad_x)) .. clamp(floor(max(..) + pad_x)), the same on y; every face entered in every
 *      cell of that rectangle is tested with THE INTERSECTION and the tie rule.  No "the hit lies in this cell" test: the minimum is
 *      idempotent, a face met twice is harmless.
 * Cost: a ray whose direction lies along a cell diagonal covers two cells per axis in a slab, four cells where an exact 3-D DDA
 * (Amanatides and Woo) would visit about three in all, and span_z more slabs at the end.  That is the price of the proof.
 *
 * THE BOUND: no face the walk has not tested is accepted with t <= the result.  Proof, for a valid face F that THE INTERSECTION accepts
 * with computed t_F; M <= R bounds its |vertex - o|; barring underflow.
 *   (a) Sideways.  By watertightness the origin of the sheared plane lies in the closed exact triangle of F's float32 sheared
 *       vertices, with exact weights w >= 0, sum 1.  A computed sheared coordinate differs from the exact one of the exact vertex by
 *       at most 6 u M (u M in A[kx], 3 u M in Sx A[kz], 2 u M in the difference).  So P = sum w_i v_i, a point OF F, has exact
 *       sheared coordinates within 6 u M of 0: with s = (P_z - o_z) / d_z, the ray's point o + s d equals P on z and is within
 *       6 u M of it on x and y.
 *   (b) Where P is filed.  P lies in F's bounding box, and cell() is monotone, so on every axis cell(P_k) lies in F's range of cells:
 *       F is entered in the cell (cell(P_x), cell(P_y), cell(P_z)).  cell()'s argument as computed is r_k (1 + e), |e| <= 3 u, of
 *       magnitude at most 1025: within 2^-12 of r_k(P_k) (4.10's argument).  Hence rho_z(s) = r_z(P_z) lies in [c - 2^-12, c + 1 +
 *       2^-12], c = cell(P_z): s lies between step 4's sa and sb for that slab; and the value cell(P_x) floors lies within
 *       6 u M / size_x + 2^-12 < pad_x of rho_x(s), which lies between rho_x(sa) and rho_x(sb): cell(P_x) is in step 4's range,
 *       the clamps being the same on both sides.  The same on y.  So F IS TESTED WHEN THE WALK VISITS THE SLAB OF P.  That slab is
 *       within first .. last as far as the box goes: P is in the box, so the ray is in the padded box at s, b0 <= s <= b1.
 *   (c) Along the ray.  t_F is NOT s: with U, V, W of one sign, t_F = sum w'_i Z_i (1 + e_i), |e_i| <= 6 u, for the COMPUTED weights w'
 *       (>= 0, sum 1), Z_i = the computed Az, Bz, Cz = (v_i - o)_z / d_z (1 + 3 u).  The computed weights of a small or thin triangle
 *       far from the origin can be far from w (the edge functions cancel), so all that holds is: zeta(t_F) lies within 10 u M /
 *       size_z < pad_z of the interval F's vertices span on zeta.  The slab of P lies in the same interval, at most span_z slabs
 *       long.  So  floor(zeta(t_F) - pad_z) - span_z  <=  slab of P  <=  floor(zeta(t_F) + pad_z) + span_z.
 *   (d) tmin <= t_F gives slab of P >= floor(zeta(tmin) - pad_z) - span_z: P's slab is not in front of `first`.  If F is untested when
 *       the walk stops before slab j (step 3), or at `last` with j = last + 1, the slab of P is >= j (all earlier ones were visited),
 *       so floor(zeta(t_F) + pad_z) >= j - span_z > floor(zeta(min(tmax, best)) + pad_z): zeta(t_F) > zeta(min(tmax, best)), and
 *       zeta grows with the parameter: t_F > tmax (not accepted after all) or t_F > best -- it neither beats nor ties.  Past `last`
 *       there is no P.  Hence t and face equal the brute-force form's bit for bit, and an ANY ray is occluded in one form iff in
 *       the other.
 *
 * gpnerf_pixel_rays(cams, n_views, H, W, z_near, rays, stream): the rays through the pixel centres of calibrated cameras, rays: device
 * float [n_views][H][W][8].  cams: HOST double [n_views][21] = K 3x3 row-major, then RT 3x4 row-major, gpnerf_mesh_rasterize's layout
 * and pixel convention (the centre of pixel (column i, row j) projects to (i, j)); n_views: 1 to 8; H, W: 1 to 16384.  Float64, unfused,
 * rounded once to float32:
 *   - on the host, inv(M) of a 3x3 M = (m0 .. m8, row-major) = adj / det with adj = (m4 m8 - m5 m7, m2 m7 - m1 m8, m1 m5 - m2 m4;
 *     m5 m6 - m3 m8, m0 m8 - m2 m6, m2 m3 - m0 m5;  m3 m7 - m4 m6, m1 m6 - m0 m7, m0 m4 - m1 m3) and det = (m0 adj0 + m1 adj3) + m2 adj6;
 *     Ki = inv(K), Ri = inv(R), R = RT's left 3x3, T its last column;  o_a = -((Ri[a][0] T0 + Ri[a][1] T1) + Ri[a][2] T2);
 *   - per pixel, one lane each: c_r = (Ki[r][0] i + Ki[r][1] j) + Ki[r][2];  u = c0 / c2, v = c1 / c2;  d_a = (Ri[a][0] u + Ri[a][1] v)
 *     + Ri[a][2];  the row is (float(o), float(d), float(z_near), +inf).
 * The direction's camera-z component is 1, so t is camera z: gpnerf_mesh_rasterize's depth.  One launch.  GPNERF_E_ARG, before any
 * device call: null cams or rays, n_views outside 1..8, H or W outside 1..16384, a z_near that is not > 0 and finite, a K or R whose
 * det is 0 or not finite. */
#define GPNERF_RAYCAST_NEAREST 0
#define GPNERF_RAYCAST_ANY 1
#define GPNERF_RAYCAST_MAX_VIEWS 8
int gpnerf_mesh_raycast(const float* rays, int64_t n_rays, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                        void* grid_workspace, int32_t mode, float* t, int32_t* face, float* bary, void* stream);
int gpnerf_pixel_rays(const double* cams, int32_t n_views, int32_t H, int32_t W, double z_near, float* rays, void* stream);

/* ---- colouring points from calibrated views (gpnerf_texture.hip): the colour the photographs give a mesh's vertices (or any list of
 * points), with the views in which a point is behind the camera, outside the image, off the mask, facing away or hidden by the mesh
 * left out.  Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments
 * alone; no float atomic (integer sums for the counts, one add per wavefront and counter); the call captures into a HIP graph and
 * replays with the same bytes; the result is a function of the inputs alone.
 *
 * gpnerf_texture_points(points, n_points, normals, cams, n_views, images, H, W, C, masks, vertices, n_vertices, faces, n_faces,
 * grid_workspace, z_near, cos_min, sharpness, eps, mode, fallback, background, workspace, workspace_bytes, color, weight, views, stats,
 * totals, stream):
 *   points: device float [n_points][3];  normals: device float [n_points][3] or NULL, need not be unit length;  cams: HOST double
 *   [n_views][21] = K 3x3 row-major, then RT 3x4 row-major, gpnerf_mesh_rasterize's layout; n_views: 1 to 8;  images: device float
 *   [n_views][H][W][C], channels last, C in 1..4 (GpnerfFrame.imgs as it is, C = 4; 16-byte aligned when C = 4), H, W: 1 to 16384;
 *   masks: device uint8 [n_views][H][W] (get_mask: 0, 1 and the border band's 100) or NULL;  the mesh that occludes: vertices, faces and
 *   grid_workspace as gpnerf_mesh_raycast takes them (a NULL grid selects its brute-force form), n_faces == 0: no occlusion test (a
 *   grid is then refused);  fallback: device float [n_points][C] or NULL;  background: HOST float [C].
 *
 * THE DEFINITION.  All arithmetic float64, multiply then add, unfused, in the order written, rounded to float32 once at the end.
 * Per (point p, view): the FIRST rule that applies names the pair's fate; every pair has exactly one.
 *   1. BEHIND.  gpnerf_mesh_rasterize's projection of a vertex: the float32 point widened to float64, c = p0 RT[:,0] + p1 RT[:,1] + p2
 *      RT[:,2] + RT[:,3], h = c0 K[:,0] + c1 K[:,1] + c2 K[:,2], z = h2, x = h0 / h2, y = h1 / h2.  BEHIND unless x, y and z are
 *      finite and z >= z_near.
 *   2. OUTSIDE unless 0 <= x <= W - 1 and 0 <= y <= H - 1: pixel centres are at integer coordinates (the rasteriser's convention,
 *      grid_sample's align_corners=True), so the image's frame is the hull of its pixel centres.
 *   3. MASKED (masks given) unless the mask at row rint(y), column rint(x) (half to even) is exactly 1.
 *   4. BACKFACING (normals given).  e = the view's eye, e_a = -((RT[0][a] RT[0][3] + RT[1][a] RT[1][3]) + RT[2][a] RT[2][3]) (-R^T T)
 *      in float64 on the host, rounded to float32.  v = e - p in float32 (one rounding per component), widened.  a = (n0 v0 + n1 v1)
 *      + n2 v2, nn = (n0 n0 + n1 n1) + n2 n2, vv likewise.  BACKFACING unless nn is finite, a > 0 and a a >= ((cos_min cos_min) nn) vv
 *      (cos_min cos_min formed on the host): a zero or non-finite normal is BACKFACING.  The weight: r = (a a) / (nn vv), w = r
 *      multiplied by r (sharpness - 1) times; sharpness 0: w = 1.  Without normals there is no facing test and w = 1.
 *   5. OCCLUDED (n_faces > 0).  The row (o = p, d = v, tmin = eps, tmax = 1) -- mesh_visibility's row for this point and eye -- goes
 *      through gpnerf_mesh_raycast in GPNERF_RAYCAST_ANY mode; OCCLUDED unless its t > 0 (t = 0: a face lies between; t = NaN: a row
 *      that is not a ray, e.g. a v that overflowed, or a grid that is not OK -- mesh_visibility's answer in every case).
 *   6. USED.  The colour is the bilinear sample: i0 = floor(x), i1 = min(i0 + 1, W - 1), fx = x - i0, the same for j0, j1, fy from y;
 *      with cab = image[view][row jb][column ia], per channel top = c00 (1 - fx) + c10 fx, bottom = c01 (1 - fx) + c11 fx,
 *      colour = top (1 - fy) + bottom fy.
 * Per point:
 *   - GPNERF_TEXTURE_BLEND: S = 0, D = 0; over the USED views in ascending index S = S + w colour (per channel), D = D + w;
 *     color = float(S / D), weight = float(D), views = the USED views' bits;
 *   - GPNERF_TEXTURE_BEST: the USED view of the largest w, the lowest index among equal w; color = float(its colour), weight =
 *     float(its w), views = its bit alone;
 *   - no USED view: color = the point's fallback row, or background without one; weight = 0, views = 0.
 * Outputs, each optional (NULL): color device float [n_points][C]; weight device float [n_points]; views device uint8 [n_points], bit
 * v set iff view v was USED (BEST: the chosen one);  stats device int64 [n_views][GPNERF_TEXTURE_FATES], the pairs of each view under
 * their fate (GPNERF_TEXTURE_USED ... _OCCLUDED; a row sums to n_points; BEST counts every USED pair, chosen or not);  totals device
 * int64 [2]: the points with at least one USED view, and those with none.  The call sets stats and totals.
 * Launches: (a) prepare, one lane per point, the views in a loop: rules 1-4, the pair's fate, weight and row into the workspace -- a
 * pair that is already decided gets the row (0, 0, 0; 0, 0, 1; tmin 1, tmax 0), which gpnerf_mesh_raycast rejects as "not a ray"
 * without a walk; block 0 zeroes stats and totals;  (b) with n_faces > 0, gpnerf_mesh_raycast itself over the [n_points][n_views] rows
 * (its one or two launches);  (c) blend, one lane per point: the cast's answer, the taps (C = 4: one 16-byte load each), the blend,
 * the outputs and the counts.  n_points == 0: (a) alone.
 * workspace: gpnerf_texture_workspace_bytes(n_points, n_views) bytes (host arithmetic only; 0 for what the call refuses), 16-byte
 * aligned, = align256(32 P) + align256(4 P) + align256(4 P) + align256(8 P) + align256(P), P = n_points n_views: the rows, the
 * cast's t and face, the weights (float64), the fates.  It carries nothing from call to call.
 * GPNERF_E_ARG, before anything is launched: null cams, images, background or workspace; null points with n_points > 0; n_points
 * negative or >= 2^31; n_views outside 1..8; H or W outside 1..16384; C outside 1..4; images not 16-byte aligned with C = 4; a z_near
 * that is not > 0 and finite; cos_min outside [0, 1) or NaN; sharpness outside 0..4; eps outside [0, 1] or NaN; a mode that is
 * neither of the two; n_faces negative or >= 2^31; n_faces > 0 with null vertices or faces or n_vertices < 0; a grid with n_faces ==
 * 0; a workspace under the formula or not 16-byte aligned. */
#define GPNERF_TEXTURE_BLEND 0
#define GPNERF_TEXTURE_BEST 1
#define GPNERF_TEXTURE_USED 0
#define GPNERF_TEXTURE_BEHIND 1
#define GPNERF_TEXTURE_OUTSIDE 2
#define GPNERF_TEXTURE_MASKED 3
#define GPNERF_TEXTURE_BACKFACING 4
#define GPNERF_TEXTURE_OCCLUDED 5
#define GPNERF_TEXTURE_FATES 6
#define GPNERF_TEXTURE_MAX_VIEWS 8
#define GPNERF_TEXTURE_MAX_SHARPNESS 4
size_t gpnerf_texture_workspace_bytes(int64_t n_points, int32_t n_views);
int gpnerf_texture_points(const float* points, int64_t n_points, const float* normals, const double* cams, int32_t n_views,
                          const float* images, int32_t H, int32_t W, int32_t C, const uint8_t* masks, const float* vertices,
                          int64_t n_vertices, const int32_t* faces, int64_t n_faces, void* grid_workspace, double z_near, double cos_min,
                          int32_t sharpness, float eps, int32_t mode, const float* fallback, const float* background, void* workspace,
                          size_t workspace_bytes, float* color, float* weight, uint8_t* views, int64_t* stats, int64_t* totals,
                          void* stream);

/* ---- a per-face texture atlas (gpnerf_atlas.hip): every face owns a triangular lattice of texels on its own surface, two faces share
 * a rectangular cell of the atlas image.  There is no unwrap: the parameterisation is host arithmetic on the face index.  The texels'
 * surface points go through gpnerf_texture_points UNCHANGED -- a texel's colour, weight, view bits and fate are by definition what that
 * call gives its point and normal --, the colour list is packed into the image, and the mesh is drawn from the image over
 * gpnerf_mesh_rasterize's face ids.  All device entry points: kernel launches only, on the caller's stream; nothing allocated, nothing
 * waited for; every launch sized from the arguments alone; no atomic, no host read; every call captures into a HIP graph and replays
 * with the same bytes; the result is a function of the inputs alone.  All arithmetic float64, multiply then add, unfused, in the order
 * written, rounded to float32 once.
 *
 * THE DEFINITION, 1: the parameterisation.  R = res, the texels along a face edge, 2 <= R <= 64.
 *   - face f with corners (a, b, c) owns the texels (i, j), i >= 0, j >= 0, i + j <= R - 1: tpf = R (R + 1) / 2 of them; texel (i, j)
 *     has the index t = j R - j (j - 1) / 2 + i within its face (rows of j, i ascending) and the global number f tpf + t;
 *   - its weights are wb = double(i) / double(R - 1), wc = double(j) / double(R - 1), wa = double(R - 1 - i - j) / double(R - 1): corner a
 *     is texel (0, 0), b is (R - 1, 0), c is (0, R - 1), so the corner texels are the vertices bit for bit;
 *   - packing: faces 2q and 2q + 1 share cell q, R + 2 texels wide and R high.  Face 2q's texel (i, j) sits at cell-local (x, y) =
 *     (i, j) (x + y <= R - 1), face 2q + 1's at (R + 1 - i, R - 1 - j) (x + y >= R + 1); the diagonal x + y = R is the GUTTER between
 *     the two hypotenuses.  P = ceil(n_faces / 2) cells, Cx = the smallest integer with Cx Cx >= P, Cy = ceil(P / Cx) (0 cells: 0 by
 *     0); cell q sits at column q % Cx and row q / Cx.  The image is Wt = Cx (R + 2) wide and Ht = Cy R high, row 0 at the top;
 *   - the UV of the texel at image column X, row Y is u = (X + 0.5) / Wt, v = 1 - (Y + 0.5) / Ht (OBJ's v points up).  A bilinear
 *     sampler that stays inside a face's UV triangle reads other data only on the gutter along the hypotenuse.
 * gpnerf_atlas_layout(n_faces, res, layout): HOST only.  layout: HOST int64 [GPNERF_ATLAS_LAYOUT_INTS] = Cx, Cy, Wt, Ht, tpf and
 * n_faces tpf (GPNERF_ATLAS_CELLS_X ... _N_TEXELS).  GPNERF_E_ARG: a null layout, res outside 2..64, n_faces negative or >= 2^31, Wt
 * or Ht above 16384, 2^31 texels or more.  Every call below refuses what this one refuses, before anything is launched.
 *
 * THE DEFINITION, 2: gpnerf_atlas_texels(vertices, n_vertices, faces, n_faces, normals, attrs, C, res, first_face, n_faces_here,
 * points, out_normals, out_attrs, stream): the texels of the faces first_face .. first_face + n_faces_here - 1, T = n_faces_here tpf
 * rows in global texel order.  normals: device float [n_vertices][3] or NULL; attrs: device float [n_vertices][C], C in 1..4, or NULL.
 * Outputs, each optional (NULL):
 *   - points device float [T][3] = float((wa a + wb b) + wc c) per component, the float32 corners widened;
 *   - out_normals device float [T][3]: the same combination of the corners' normals; without normals the face's (b - a) x (c - a) --
 *     u = b - a, v = c - a, (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0) in float64, rounded, not normalised (what rule 4 of
 *     gpnerf_texture_points accepts) -- for every texel of the face;
 *   - out_attrs device float [T][C]: the same combination of the corners' attributes.
 * A face that names a vertex outside [0, n_vertices) gives NaN in every output row of its texels (gpnerf_texture_points files a NaN
 * point as BEHIND in every view).  One launch, a lane per texel; T == 0 or no output: none.  GPNERF_E_ARG: the layout's refusals; null
 * vertices with n_vertices > 0 or faces with n_faces > 0, n_vertices negative or >= 2^31; first_face or n_faces_here negative or
 * first_face + n_faces_here > n_faces; C outside 1..4 with attrs or out_attrs; out_attrs without attrs (n_vertices > 0).
 *
 * THE DEFINITION, 4: gpnerf_atlas_pack(colors, views, n_faces, res, C, background, atlas, coverage, stream): colors: device float
 * [n_faces tpf][C], the colour list in global texel order; views: device uint8 [n_faces tpf] (gpnerf_texture_points' view bits) or
 * NULL (every texel counts as seen); background: HOST float [C].  Outputs, each optional: atlas device float [Ht][Wt][C], coverage
 * device uint8 [Ht][Wt].  Every image texel inverts the packing: with q = (Y / R) Cx + X / (R + 2), x = X % (R + 2), y = Y % R,
 *   - q >= P: GPNERF_ATLAS_UNOWNED (0), the texel takes background;
 *   - x + y == R: GPNERF_ATLAS_GUTTER (3).  It takes the float64 sum of its left, upper, right and lower neighbours' colours, in that
 *     order, over those that lie in the image and are owned, divided by double(their number); background when there are none (no
 *     neighbour of a gutter texel is a gutter texel);
 *   - otherwise the face is 2q (x + y < R, (i, j) = (x, y)) or 2q + 1 ((i, j) = (R + 1 - x, R - 1 - y)); a face >= n_faces (the absent
 *     odd face): UNOWNED; else the texel takes its row of colors, coverage GPNERF_ATLAS_SEEN (1) where its view bits are not 0 and
 *     GPNERF_ATLAS_FALLBACK (2) where they are.
 * One launch, a lane per image texel: a gather, no clear pass and no scatter.  GPNERF_E_ARG: the layout's refusals; a null background;
 * null colors with texels; C outside 1..4.
 *
 * THE DEFINITION, 5: gpnerf_atlas_shade(face_id, vertices, n_vertices, faces, n_faces, cams, n_views, H, W, z_near, atlas, res, C,
 * filter, background, out, stream): face_id, the mesh, cams, n_views, H, W, z_near and background as gpnerf_mesh_interpolate takes
 * them; atlas: device float [Ht][Wt][C] for (n_faces, res); out: device float [n_views][H][W][C].  A pixel is shaded where its face_id
 * names a face that is drawn in that view and covers it -- gpnerf_mesh_interpolate's condition, its Ek, wk, zk, q and uk recomputed
 * exactly as there --; every other pixel takes background.  With clamp(v, lo, hi) = (v > lo ? v : lo) then (v < hi ? v : hi):
 *   s = clamp(ub (R - 1), 0, R - 1), t = clamp(uc (R - 1), 0, (R - 1) - s), i0 = min(int(floor(s)), R - 1), j0 = min(int(floor(t)),
 *   R - 1 - i0), fs = s - i0, ft = t - j0.
 *   - GPNERF_ATLAS_SIMPLEX: in the lower half-cell (fs + ft <= 1, or i0 + j0 >= R - 2) the taps are (i0, j0) with weight (1 - fs) - ft,
 *     (i0 + 1, j0) with fs and (i0, j0 + 1) with ft; otherwise (i0 + 1, j0) with 1 - ft, (i0, j0 + 1) with 1 - fs and (i0 + 1, j0 + 1)
 *     with (fs + ft) - 1.  A tap with i + j > R - 1 is NOT READ and its weight is dropped.  S = 0, D = 0; over the read taps in the
 *     order (0,0), (1,0), (0,1), (1,1) of (i - i0, j - j0): S = S + w colour (per channel), D = D + w; out = float(S / D);
 *   - GPNERF_ATLAS_NEAREST: the colour of the read tap of the largest weight, the first in that order among equal weights.
 * The texel (i, j) of face f is read at its image position (the packing above): only the face's own texels, never a neighbour cell,
 * never the gutter.  One launch, a lane per pixel and view.  GPNERF_E_ARG: the layout's refusals; what gpnerf_mesh_interpolate refuses
 * of the arguments they share; a null atlas with n_faces > 0; C outside 1..4; a filter that is neither of the two.
 * Known limit: the texel density is uniform per FACE, not per area -- right for marching-cubes and vertex-clustered meshes, whose
 * faces are near-uniform in size, wasteful for arbitrary scans. */
#define GPNERF_ATLAS_CELLS_X 0
#define GPNERF_ATLAS_CELLS_Y 1
#define GPNERF_ATLAS_WIDTH 2
#define GPNERF_ATLAS_HEIGHT 3
#define GPNERF_ATLAS_TEXELS_PER_FACE 4
#define GPNERF_ATLAS_N_TEXELS 5
#define GPNERF_ATLAS_LAYOUT_INTS 6
#define GPNERF_ATLAS_UNOWNED 0
#define GPNERF_ATLAS_SEEN 1
#define GPNERF_ATLAS_FALLBACK 2
#define GPNERF_ATLAS_GUTTER 3
#define GPNERF_ATLAS_SIMPLEX 0
#define GPNERF_ATLAS_NEAREST 1
#define GPNERF_ATLAS_MIN_RES 2
#define GPNERF_ATLAS_MAX_RES 64
int gpnerf_atlas_layout(int64_t n_faces, int32_t res, int64_t* layout);
int gpnerf_atlas_texels(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* normals,
                        const float* attrs, int32_t C, int32_t res, int64_t first_face, int64_t n_faces_here, float* points,
                        float* out_normals, float* out_attrs, void* stream);
int gpnerf_atlas_pack(const float* colors, const uint8_t* views, int64_t n_faces, int32_t res, int32_t C, const float* background,
                      float* atlas, uint8_t* coverage, void* stream);
int gpnerf_atlas_shade(const int32_t* face_id, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                       const double* cams, int32_t n_views, int32_t H, int32_t W, double z_near, const float* atlas, int32_t res, int32_t C,
                       int32_t filter, const float* background, float* out, void* stream);

/* ---- fusing depth maps into a truncated signed distance field (gpnerf_fusion.hip): Curless and Levoy's volumetric integration of
 * calibrated depth maps -- a radiance field's rendered depth, gpnerf_mesh_rasterize's, a sensor's -- on a lattice.  Marching cubes at
 * the field's zero is the fused surface.  Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every
 * launch sized from the arguments alone; no float atomic (integer sums for the counts, into counters a kernel of the library's own
 * zeroes: no memset node); every call captures into a HIP graph and replays with the same
 * bytes; the result is a function of the inputs alone.
 *
 * The lattice: dims = (nx, ny, nz) POINTS at lo + (i, j, k) * step, lattice HOST double [6] = lo, step: gpnerf_mesh_sdf's layout and
 * limits (each dims entry >= 1, the product <= 2^28), z fastest in memory.  cams: HOST double [n_views][21] = K 3x3 row-major, then RT
 * 3x4 row-major, gpnerf_mesh_rasterize's layout; n_views: 1 to 8.  depth: device float [n_views][H][W], CAMERA Z -- gpnerf_mesh_rasterize's
 * depth, and gpnerf_mesh_raycast's t along gpnerf_pixel_rays' rays; H, W: 1 to 16384.  weights: device float [n_views][H][W], or NULL:
 * every weight 1.  band: float, finite, > 0, at most 1024 x the smallest step (gpnerf_mesh_sdf's rule).  z_near: > 0 and finite.
 * carve: 0 or 1.
 *
 * THE DEFINITION (gpnerf_fusion_integrate).  All arithmetic float64, multiply then add, unfused, in the order written.
 * Per (lattice point p, view): the FIRST rule that applies names the pair's fate; every pair has exactly one.
 *   1. BEHIND.  p_a = float32(lo_a + double(i_a) * step_a) (product and sum in float64, one rounding), widened to float64;
 *      gpnerf_mesh_rasterize's projection of a vertex (gpnerf_texture_points, rule 1): c = p0 RT[:,0] + p1 RT[:,1] + p2 RT[:,2] +
 *      RT[:,3], h = c0 K[:,0] + c1 K[:,1] + c2 K[:,2], z = h2, x = h0 / h2, y = h1 / h2.  BEHIND unless x, y and z are finite and z >=
 *      z_near.
 *   2. OUTSIDE unless 0 <= x <= W - 1 and 0 <= y <= H - 1 (pixel centres at integer coordinates).
 *   3. NODATA.  d = depth[view][row rint(y)][column rint(x)] (half to even) and w = the weight there (1 without weights): the NEAREST
 *      pixel, never a bilinear tap -- a tap across a silhouette would mix +inf into a surface.  NODATA if d is NaN, -inf or <= 0; if w
 *      is not finite or not > 0; if d = +inf with carve = 0.
 *   4. EMPTY (background): d = +inf with carve = 1 -- the pixel sees past everything; t = band.
 *   5. HIDDEN.  s = d - z (d widened).  HIDDEN if s < -band: the pair contributes nothing; bit 0 (GPNERF_FUSION_FLAG_HIDDEN) of the
 *      point's flag byte is set.
 *   6. EMPTY (in front): s >= band; t = band.
 *   7. NEAR otherwise; t = s; bit 1 (GPNERF_FUSION_FLAG_NEAR) of the flag byte is set.
 * The EMPTY and NEAR pairs of a point contribute in ascending view index: sum = sum + w t, then weight = weight + w.
 * State, [nx][ny][nz] each: sum and weight device double, flags device uint8.  gpnerf_fusion_reset zeroes it; an integrate call
 * CONTINUES the sums it is handed, so views 0..7 in one call and views 0..3 then 4..7 in two leave the same bits: that is how more
 * than eight views are fused.
 * Finalise (gpnerf_fusion_finalise), per point: weight > 0: value = float32(sum / weight), clamped to [-band, band]; otherwise, bit 0
 * of the flags set: value = -band (unseen, and behind a surface in some view: interior); otherwise value = +band (unknown reads as
 * empty).  gpnerf_mesh_sdf's convention: negative inside, +-band where flat.
 * Counts.  stats: device int64 [n_views][GPNERF_FUSION_FATES], the pairs of each view of THE CALL under their fate (a row sums to
 * nx ny nz); integrate and oneshot set it.  totals: device int64 [GPNERF_FUSION_TOTALS], set by finalise and oneshot: the points with
 * weight > 0 (SEEN), with the NEAR bit (SURFACE), interior-filled (INTERIOR), unknown (UNKNOWN); SEEN + INTERIOR + UNKNOWN = nx ny nz.
 * gpnerf_fusion_oneshot is reset + integrate + finalise of at most eight views in one pass, the sums in registers: sdf, flags (or
 * NULL), stats and totals EQUAL those three calls' bit for bit; the state is never written.
 * Launches: reset: one; integrate: the counters' clear (one wavefront) and a sweep over the lattice by at most 768 blocks of 512 lanes,
 * one lattice point per lane and step, consecutive lanes consecutive k, the views in a loop inside the lane, the cameras in the kernel
 * argument (scalar loads): one load and one store of the 17-byte state per point; finalise: the clear and the same sweep; oneshot: the
 * clear and the integrate kernel's other instantiation.  The counts: one integer add per wavefront and counter into the block's LDS,
 * one per block and counter into memory when the block has swept its share.
 * GPNERF_E_ARG, before anything is launched: a null depth, cams, lattice, dims, sum, weight, flags (oneshot: flags may be NULL), sdf,
 * stats or totals where the call takes it; a dims entry < 1 or a product > 2^28; n_views outside 1..8; H or W outside 1..16384; a band
 * that is NaN, infinite, <= 0 or above 1024 x the smallest step (finalise, which has no lattice: NaN, infinite or <= 0); a z_near
 * that is not > 0 and finite; carve neither 0 nor 1; a lattice entry that is not finite or a step that is not > 0. */
#define GPNERF_FUSION_BEHIND 0
#define GPNERF_FUSION_OUTSIDE 1
#define GPNERF_FUSION_NODATA 2
#define GPNERF_FUSION_EMPTY 3
#define GPNERF_FUSION_HIDDEN 4
#define GPNERF_FUSION_NEAR 5
#define GPNERF_FUSION_FATES 6
#define GPNERF_FUSION_SEEN 0
#define GPNERF_FUSION_SURFACE 1
#define GPNERF_FUSION_INTERIOR 2
#define GPNERF_FUSION_UNKNOWN 3
#define GPNERF_FUSION_TOTALS 4
#define GPNERF_FUSION_FLAG_HIDDEN 1
#define GPNERF_FUSION_FLAG_NEAR 2
#define GPNERF_FUSION_MAX_VIEWS 8
int gpnerf_fusion_reset(const int32_t* dims, double* sum, double* weight, uint8_t* flags, void* stream);
int gpnerf_fusion_integrate(const float* depth, const float* weights, const double* cams, int32_t n_views, int32_t H, int32_t W,
                            const double* lattice, const int32_t* dims, float band, double z_near, int32_t carve, double* sum,
                            double* weight, uint8_t* flags, int64_t* stats, void* stream);
int gpnerf_fusion_finalise(const double* sum, const double* weight, const uint8_t* flags, const int32_t* dims, float band, float* sdf,
                           int64_t* totals, void* stream);
int gpnerf_fusion_oneshot(const float* depth, const float* weights, const double* cams, int32_t n_views, int32_t H, int32_t W,
                          const double* lattice, const int32_t* dims, float band, double z_near, int32_t carve, float* sdf, uint8_t* flags,
                          int64_t* stats, int64_t* totals, void* stream);

/* ---- per-frame sparse convolution pyramid (gpnerf_volume.hip), replacing the external spconv v1.2.1 calls of
 * libs/nerfheads/networks/SparseConvNet.py:22-111 (SubMConv3d / SparseConv3d + BatchNorm1d + ReLU, .dense()).
 * A sparse tensor is: features [M][C] fp32, coords [M][3] int32 (d,h,w), and a dense int32 index grid [D][H][W]
 * (row of the site, -1 = inactive).  Row counts may live on the device (m_dev, NULL = use m_cap) so a chain of levels
 * needs no host synchronisation; m_cap bounds every launch.  All pointers device unless noted; dims: host int32[3].
 * Parity unpinned: spconv is not in the reference tree. */
/* grid <- -1, then grid[coords[i]] = i (highest row wins for duplicate voxels). */
int gpnerf_sparse_index(const int32_t* coords, const int32_t* m_dev, int32_t m_cap, const int32_t* dims, int32_t* grid,
                        void* stream);
/* 3x3x3 conv + folded BatchNorm + ReLU over the sites listed in out_coords.
 * strided = 0: submanifold (SubMConv3d; in/out share sites and grid), strided = 1: SparseConv3d(k=3, s=2, p=1) reading
 * the finer level (in_grid/in_dims) at the coarser sites of out_coords.  weight [27][cin][cout] (spconv's [3,3,3,Ci,Co]). */
int gpnerf_sparse_conv3(int32_t strided, const float* in, int32_t cin, const int32_t* in_grid, const int32_t* in_dims,
                        const int32_t* out_coords, const int32_t* m_dev, int32_t m_cap, const float* weight, int32_t cout,
                        const float* bn_scale, const float* bn_shift, float* out, void* stream);
/* The same convolution on the matrix cores (32 output sites per wavefront, v_mfma_f32_32x32x2_f32; cin a multiple of 8,
 * cin, cout <= 32).  packed_weight: device copy of gpnerf_sparse_pack_weight()'s image of the [27][cin][cout] weight
 * (host side, model-load time; gpnerf_sparse_packed_weight_floats(cin) floats).  Same result as gpnerf_sparse_conv3 up to
 * fp32 summation order. */
int64_t gpnerf_sparse_packed_weight_floats(int32_t cin);
int gpnerf_sparse_pack_weight(const float* weight_host, int32_t cin, int32_t cout, float* packed_host);
int gpnerf_sparse_conv3_mfma(int32_t strided, const float* in, int32_t cin, const int32_t* in_grid, const int32_t* in_dims,
                             const int32_t* out_coords, const int32_t* m_dev, int32_t m_cap, const float* packed_weight,
                             int32_t cout, const float* bn_scale, const float* bn_shift, float* out, void* stream);
/* The same convolution in the encoder's split-precision arithmetic (cin = 16 or 32, cout <= 32): every fp32 operand as f16 hi + lo,
 * three v_mfma_f32_32x32x16_f16 per 16 input channels, f32 accumulation -- the fp32 matrix instruction above runs at 1/16 of the
 * f16 rate.  packed_weight16: device copy of gpnerf_sparse_pack_weight16()'s image (host side, model-load time;
 * gpnerf_sparse_packed_weight16_bytes(cin) bytes; refuses |w| >= 15.99): per (tap, 16-channel chunk) the scaled weights as f16
 * hi | lo and once more in fp32.  A wavefront that gathers a value beyond the f16 range (|x| >= 4 094) runs that tap on the fp32
 * instructions with the fp32 copy.  Within 2^-21 (relative to the sum of |terms|) of gpnerf_sparse_conv3_mfma. */
int64_t gpnerf_sparse_packed_weight16_bytes(int32_t cin);
int gpnerf_sparse_pack_weight16(const float* weight_host, int32_t cin, int32_t cout, void* packed_host);
int gpnerf_sparse_conv3_mfma16(int32_t strided, const float* in, int32_t cin, const int32_t* in_grid, const int32_t* in_dims,
                               const int32_t* out_coords, const int32_t* m_dev, int32_t m_cap, const void* packed_weight16,
                               int32_t cout, const float* bn_scale, const float* bn_shift, float* out, void* stream);
/* The whole pyramid of SparseConvNet.py:90-111 behind two calls (the entries above, in the reference's order, enqueued from
 * native code: ~60 launches without a trip through the host language between them).  The caller owns every buffer.
 *   gpnerf_sparse_pyramid_plan: everything that depends on the vertices' voxel coordinates only -- the full-resolution index grid,
 *     every coarse level's site list + grid (gpnerf_sparse_down_sites) and the zeroed dense volumes; may run on another stream
 *     beside the image encoder.
 *   gpnerf_sparse_pyramid_run: double_conv at full resolution, the duplicate merge, then per level strided conv + double_conv +
 *     scatter into vol[i] (channels-last [D_i][H_i][W_i][ch_i]).  convs: 2 + 3 * n_levels entries in network order.
 * feat_a / feat_b: two float buffers of max(m0, cap[i]) * 32 each (ping-pong).  code: [m0][code_ch] per-vertex features.
 * Rows that share a voxel (two vertices rounded into one 5 mm cell) follow spconv v1.2.1's rulebook as oracle/producers_ref.py's
 * header recalls it: a submanifold convolution gives the voxel's OWNER row (the highest) the sum over ALL rows of its neighbour
 * voxels and every other row of the voxel only its own centre term; a strided convolution takes every row. */
#define GPNERF_PYRAMID_MAX_LEVELS 4
typedef struct GpnerfSparseConv {
    int32_t strided, cin, cout;
    int32_t form;                 /* 2: gpnerf_sparse_conv3_mfma16 (weight = its packed image), 1: _mfma, 0: gpnerf_sparse_conv3 (raw [27][cin][cout]) */
    const void* weight;
    const float* bn_scale;
    const float* bn_shift;
    const float* weight_raw;      /* device [27][cin][cout] fp32, spconv's own layout: needed for the two vertex-level convolutions
                                     (rows that share a voxel are recomputed from it), may be NULL for the others */
} GpnerfSparseConv;
typedef struct GpnerfPyramid {
    int32_t n_levels, m0;
    int32_t dims0[3];
    int32_t dims[GPNERF_PYRAMID_MAX_LEVELS][3];
    int32_t cap[GPNERF_PYRAMID_MAX_LEVELS];
    int32_t ch[GPNERF_PYRAMID_MAX_LEVELS];
    const int32_t* coords0;       /* [m0][3] (d, h, w) */
    int32_t* grid0;               /* dims0 cells */
    int32_t* dup_scratch;         /* 9 * m0 */
    int32_t* grid[GPNERF_PYRAMID_MAX_LEVELS];
    int32_t* coords[GPNERF_PYRAMID_MAX_LEVELS];     /* [cap][3] */
    int32_t* m[GPNERF_PYRAMID_MAX_LEVELS];          /* device row counts */
    float* vol[GPNERF_PYRAMID_MAX_LEVELS];
    float* feat_a;
    float* feat_b;
    float* feat_c;                /* m0 * 32 floats: the vertex level's input with every shared voxel's rows summed into its owner */
} GpnerfPyramid;
int gpnerf_sparse_pyramid_plan(const GpnerfPyramid* p, void* stream);
int gpnerf_sparse_pyramid_run(const GpnerfPyramid* p, const float* code, int32_t code_ch, const GpnerfSparseConv* convs, int32_t n_convs,
                              void* stream);
/* Before the first strided conv: feat[owner] += feat[i] for every row i whose voxel is indexed by another row (two
 * vertices rounded into one voxel).  spconv's strided rulebook takes every input row; its submanifold lookups one.
 * The rows of a voxel are added in ascending row order (deterministic); scratch: device int32[9 * m], overwritten (a count
 * and eight row slots per row). */
int gpnerf_sparse_merge_duplicates(float* feat, int32_t channels, const int32_t* coords, const int32_t* grid, int32_t m,
                                   const int32_t* dims, int32_t* scratch, void* stream);
/* Active sites of the next (half-resolution) level: out_grid / out_coords / m_out_dev from the finer level's coords. */
int gpnerf_sparse_down_sites(const int32_t* in_coords, const int32_t* m_in_dev, int32_t m_in_cap, const int32_t* out_dims,
                             int32_t* out_grid, int32_t* out_coords, int32_t* m_out_dev, int32_t m_out_cap, void* stream);
/* .dense(): zero-filled [D][H][W][C] volume with the active sites' features (channels-last, as GpnerfFrame.vol wants). */
int gpnerf_sparse_to_dense(const float* feat, int32_t channels, const int32_t* coords, const int32_t* grid, const int32_t* m_dev,
                           int32_t m_cap, const int32_t* dims, float* vol_ndhwc, void* stream);
/* The same in two steps, for callers that lay out a frame's pyramid BEFORE its features exist (the structure of the pyramid --
 * index grids, coarse site lists, zeroed dense volumes -- depends on the vertices' voxel coordinates only, so it can be enqueued
 * on a side stream while the image encoder runs): gpnerf_zero_volume now, gpnerf_sparse_scatter_dense(prezeroed = 1) later. */
int gpnerf_zero_volume(float* vol_ndhwc, int32_t channels, const int32_t* dims, void* stream);
int gpnerf_sparse_scatter_dense(const float* feat, int32_t channels, const int32_t* coords, const int32_t* grid, const int32_t* m_dev,
                                int32_t m_cap, const int32_t* dims, float* vol_ndhwc, int32_t prezeroed, void* stream);

/* Vertex-code attention of the volume builder (libs/nerfheads/trainhead.py:48-52, networks/MultiHeadAttention.py:61-98 with
 * sum=False): q [n][d_model] vertex codes, kv [n][views][kv_dim] the vertices' per-view features, weights in PyTorch
 * layout (w_qs [d_model][d_model], w_ks / w_vs [d_model][kv_dim], fc [d_model][d_model]); out [n][d_model].  All device.
 * d_model, kv_dim <= 64, views <= 4, d_model / n_head a power of two. */
int gpnerf_vertex_attention(const float* q, const float* kv, const float* w_qs, const float* w_ks, const float* w_vs,
                            const float* fc, int32_t n, int32_t d_model, int32_t kv_dim, int32_t n_head, int32_t views,
                            float* out, void* stream);

/* The image encoder on channels-last activations (gpnerf_conv.hip), all tensors device fp32 [N][H][W][C].
 * conv2d_nhwc = nn.Conv2d(cin, cout, ks, stride, padding=ks/2, padding_mode='reflect') (UNet.py:6-14,108-115,154-155) as an
 *   implicit GEMM on the matrix cores, in one of two arithmetic forms chosen by `exact` (the SAME kernels, tiles, staging and
 *   fused InstanceNorm tables either way; `packed` must be the image gpnerf_conv_pack_weight wrote for that form):
 *     exact = 1  fp32 operands on v_mfma_f32_32x32x2_f32: every dot product an fp32 FMA chain over (channel block, tap, channel),
 *                the reference's own arithmetic up to the order of the sum; no operand range, range_flag is not looked at.  The
 *                encoder's default (ResUNet.precision = "fp32"): the end-to-end chain then stays inside 1e-4 of the reference.
 *     exact = 0  fp32 operands split into f16 hi + lo on v_mfma_f32_32x32x16_f16 (three MFMAs per k-step, f32 accumulation:
 *                ~23 bits per operand, 3/16 of the matrix time); operands must stay below the f16 range, which InstanceNorm'd /
 *                ReLU'd activations of images do -- see range_flag.  The fast mode (ResUNet.precision = "split").
 *   ks in {1, 3, 7}, stride in {1, 2}; cin a multiple of 16, or < 8 for the 7x7/2 stem; cout a multiple of 4.
 *   packed: gpnerf_conv_pack_weight()'s device image of the PyTorch weight [cout][cin][ks][ks] (gpnerf_conv_packed_bytes()
 *   bytes; re-pack when the parameter changes); bias: [cout] or NULL.  y: [N][Ho][Wo][cout], Ho = (H + 2 (ks/2) - ks) / stride + 1.
 *   tile_stats: NULL, or [N][gpnerf_conv_out_tiles()][cout][3] floats that receive every workgroup tile's per-channel sum, sum of
 *   squares, and M2 (sum of squares about the tile's own mean) of the outputs -- the statistics the InstanceNorm behind the
 *   convolution needs, without re-reading y.  out_table below takes the variance from the M2's and the spread of the tiles' means
 *   (sum s^2 / n - (sum s)^2 / hw, in double), and merges the tiles pairwise as Chan et al. on a channel whose values are nearly
 *   constant over the image.
 * instance_norm_act_nhwc = act(InstanceNorm2d(x; gamma, beta, eps, biased variance, no running statistics) [+ residual]),
 *   act 0 none / 1 ReLU / 2 ELU (UNet.py:38-53,117-120,180-183); statistics from a double-precision pass over x, added up in a
 *   fixed order (deterministic): the stand-alone operator, what the fused tables of conv2d_norm_nhwc are tested against;
 *   scratch: gpnerf_instance_norm_nhwc_scratch_bytes() bytes.
 * conv2d_norm_nhwc = conv2d_nhwc with the InstanceNorms on either side of it fused in (a residual unit is conv - norm - ReLU -
 *   conv - norm, UNet.py:38-53):
 *     in_table  NULL, or [N][3][cin] floats (mean, gamma * rstd, beta per channel, what out_table below produces): the
 *               convolution then reads act((x - mean) * scale + beta) instead of x while it stages its input, act = ReLU for
 *               in_act 1, identity for 0 -- the normalised tensor is never written.  3x3 and 1x1 convolutions with cin % 16 == 0.
 *     out_table NULL, or [N][3][cout] floats that receive mean / gamma * rstd / beta of InstanceNorm2d(y; gamma, beta, eps): the
 *               last workgroup to finish an (image, 32..64-channel group) merges that group's tile_stats rows in double, in a fixed
 *               order (deterministic), so no separate reduction launch follows the convolution.  Needs tile_stats, gamma, beta and
 *               `counters`: at least N * ceil(cout / 32) uint32 words that are zero before the call; they are zero again after it.
 * conv2d_norm_cat_nhwc = the 3x3 stride-1 convolution of conv2d_norm_nhwc on the channel concatenation [x (cin_a channels), x_b (cin_b)]
 *   of two NHWC tensors of one size (UNet.py:199-211's torch.cat([up, skip], 1) in front of iconv3 / iconv2), read in place: the
 *   concatenated tensor is never written.  cin_a, cin_b multiples of 16; `packed` is the image of the [cout][cin_a + cin_b][3][3] weight.
 * norm_apply_nhwc = act((x - mean) * scale + beta [+ residual]) from such a table; with res_table the residual is itself
 *   normalised on the fly ((residual - rmean) * rscale + rbeta: the projected shortcut's InstanceNorm, UNet.py:48-51).
 * upsample2x_nhwc = F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) (UNet.py:129).
 * range_flag (the three convolutions, exact = 0 only): NULL, or ONE uint32 word (device memory, or pinned host memory the device can
 *   write) that the call sets to 1 -- it never clears it -- when an operand was beyond what the f16 hi/lo split holds (an
 *   activation with |x| >= 4095, a weight with |w| >= 16, or a non-finite input): such an operand splits into f16 infinities and
 *   the outputs it meets are NaN, which the call finds in the sums of the InstanceNorm table (out_table given) or in its
 *   accumulators (no norm behind it).  A result produced with the flag raised must be discarded and the convolution chain run
 *   again with exact = 1 (fp32 operands, no range), so that parameters of any size are served (a trained InstanceNorm scale times sqrt(h w) can
 *   exceed the range on a one-hot image; ordinary images stay orders of magnitude below it).
 * conv2d_nhwc_exact = the same nn.Conv2d on fp32 operands (v_mfma_f32_32x32x2_f32, an fp32 FMA chain per output, any odd ks,
 *   any stride, any channel counts), from the PyTorch weight [cout][cin][ks][ks] as it is, one scalar load per operand: the
 *   independent restatement the tests hold the fused exact = 1 form against (and a way to run shapes the fused kernels do not
 *   cover); ~20x slower, not on the encoder's path.
 * conv_variant = which kernel a convolution call launches, for tools and tests.  Host arithmetic only, nothing is launched; the
 *   launchers and gpnerf_conv_out_tiles() read their choice from the same function.  n, h, w, cout, ks, stride as for
 *   conv2d_norm_nhwc with cin = cin_a and cin_b = 0, or as for conv2d_norm_cat_nhwc (cin_b > 0; ks = 3, stride = 1).
 *   variant: host, GPNERF_CONV_VARIANT_INTS int32 -- [GPNERF_CONV_FAMILY] the kernel family (GPNERF_CONV_DIRECT_1X1 ...),
 *   [GPNERF_CONV_COT] 32-channel output tiles per workgroup, [GPNERF_CONV_RW] output rows per wave of the tiled kernels (0: the
 *   direct kernel, which tiles consecutive pixels), [GPNERF_CONV_KSPLIT] halves the channel blocks are split over,
 *   [GPNERF_CONV_CAT] 1 for the concatenating form, [GPNERF_CONV_TILES] workgroup tiles per image (= gpnerf_conv_out_tiles()),
 *   [GPNERF_CONV_TILE_H], [GPNERF_CONV_TILE_W] the workgroup's tile of output pixels (tile_h = 0: tile_w consecutive pixels).
 *   Returns GPNERF_E_ARG, with the family GPNERF_CONV_REFUSED, for every shape the convolution calls refuse. */
#define GPNERF_CONV_FAMILY 0
#define GPNERF_CONV_COT 1
#define GPNERF_CONV_RW 2
#define GPNERF_CONV_KSPLIT 3
#define GPNERF_CONV_CAT 4
#define GPNERF_CONV_TILES 5
#define GPNERF_CONV_TILE_H 6
#define GPNERF_CONV_TILE_W 7
#define GPNERF_CONV_VARIANT_INTS 8
/* [GPNERF_CONV_FAMILY] */
#define GPNERF_CONV_REFUSED 0              /* the convolution calls return GPNERF_E_ARG for this shape */
#define GPNERF_CONV_DIRECT_1X1 1           /* 1x1, stride 1 or 2: the direct kernel, 256 consecutive pixels per workgroup */
#define GPNERF_CONV_DIRECT_NARROW3 2       /* 3x3 stride 1 on fewer than 8 channels: the direct kernel on the flattened (tap, channel) K */
#define GPNERF_CONV_TILED_S1 3             /* 3x3 stride 1: 4 RW rows x 32 columns per workgroup, patch staged in LDS */
#define GPNERF_CONV_TILED_S2 4             /* 3x3 stride 2: the same kernel on 4 x 32 output tiles */
#define GPNERF_CONV_STEM 5                 /* 7x7 stride 2 on at most 4 channels: 8 x 32 output tiles */
int gpnerf_conv_variant(int32_t n, int32_t h, int32_t w, int32_t cin_a, int32_t cin_b, int32_t cout, int32_t ks, int32_t stride,
                        int32_t* variant);
int64_t gpnerf_conv_packed_bytes(int32_t cout, int32_t cin, int32_t ks);
int gpnerf_conv_pack_weight(const float* weight, int32_t cout, int32_t cin, int32_t ks, int32_t exact, void* packed, void* stream);
int32_t gpnerf_conv_out_tiles(int32_t h, int32_t w, int32_t cin, int32_t ks, int32_t stride);
int gpnerf_conv2d_nhwc(const float* x, int32_t n, int32_t h, int32_t w, int32_t cin, const void* packed, const float* bias,
                       int32_t cout, int32_t ks, int32_t stride, float* y, float* tile_stats, uint32_t* range_flag, int32_t exact,
                       void* stream);
int gpnerf_conv2d_norm_cat_nhwc(const float* x, int32_t cin_a, const float* x_b, int32_t cin_b, int32_t n, int32_t h, int32_t w,
                                const void* packed, const float* bias, int32_t cout, float* y, float* tile_stats, const float* gamma,
                                const float* beta, float eps, float* out_table, uint32_t* counters, uint32_t* range_flag, int32_t exact,
                                void* stream);
int gpnerf_conv2d_norm_nhwc(const float* x, int32_t n, int32_t h, int32_t w, int32_t cin, const float* in_table, int32_t in_act,
                            const void* packed, const float* bias, int32_t cout, int32_t ks, int32_t stride, float* y, float* tile_stats,
                            const float* gamma, const float* beta, float eps, float* out_table, uint32_t* counters, uint32_t* range_flag,
                            int32_t exact, void* stream);
int gpnerf_conv2d_nhwc_exact(const float* x, int32_t n, int32_t h, int32_t w, int32_t cin, const float* weight, const float* bias,
                             int32_t cout, int32_t ks, int32_t stride, float* y, void* stream);
int gpnerf_norm_apply_nhwc(const float* x, const float* table, const float* residual, const float* res_table, int32_t n, int64_t hw,
                           int32_t c, int32_t act, float* out, void* stream);
int64_t gpnerf_instance_norm_nhwc_scratch_bytes(int32_t n, int64_t hw, int32_t c);
int gpnerf_instance_norm_act_nhwc(const float* x, const float* gamma, const float* beta,
                                  const float* residual, int32_t n, int64_t hw, int32_t c, float eps, int32_t act, float* out,
                                  void* scratch, void* stream);
int gpnerf_upsample2x_nhwc(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, float* out, void* stream);

/* Channels-last re-layouts of the per-frame tensors (device -> device). */
int gpnerf_relayout_volume(const float* ncdhw, float* ndhwc, int32_t D, int32_t H, int32_t W, void* stream);
int gpnerf_relayout_featmaps(const float* nchw, float* nhwc, int32_t V, int32_t H, int32_t W, void* stream);
/* src_imgs [V][3][H][W] in [-1,1] -> [V][H][W][4] = x*0.5+0.5 (BaseRender.py:231), 4th lane 0 */
int gpnerf_relayout_images(const float* nchw, float* nhwc4, int32_t V, int32_t H, int32_t W, void* stream);
/* Launch order of a frame's rays: order[q] = row (in the caller's ray list, which follows the raster order of the kept pixels of
 * `mask`, as ZjumocapDataset.py:505's mask_at_box does) of the q-th ray when the H x W image is walked in patches of
 * patch_w x patch_h pixels (patch_w <= 64, patch_h <= 32), patches and the pixels inside a patch in raster order -- the 32 rays of
 * a wavefront then cover a compact block (gpnerf_render_fused's ray_order).  mask: H*W bytes, non-zero = kept; n: the caller's ray
 * count; scratch: gpnerf_patch_order_scratch_bytes() bytes, overwritten.  Three launches, no host round trip; a mask that does not
 * keep exactly n pixels yields the identity 0 .. n-1.  Results of a render do not depend on the order; it is a locality choice. */
int64_t gpnerf_patch_order_scratch_bytes(int32_t H, int32_t W, int32_t patch_w, int32_t patch_h);
int gpnerf_patch_order(const uint8_t* mask, int32_t H, int32_t W, int32_t patch_w, int32_t patch_h, int32_t n, int32_t* scratch,
                       int32_t* order, void* stream);

/* Layout of the head image, for tools and tests: table[4*l + {0,1,2,3}] = k-steps, 32-row output tiles,
 * weight offset, bias offset (in floats) of MFMA layer l = GEO,D1,D2,D3,BS,BV,B2,V1,V2,R1,R2 (11 layers),
 * then table[44..47] = offsets of the 16->1 / 16->3 VALU tails (D4 weights, D4 bias, R3 weights, R3 bias).
 * table: host, 48 int32. */
int gpnerf_head_layout(int32_t* table);

const char* gpnerf_strerror(int code);
/* compile-time facts for callers / tests */
int32_t gpnerf_rays_per_tile(void);   /* rays one wavefront renders together (32) */
const char* gpnerf_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* GPNERF_HIP_H */
