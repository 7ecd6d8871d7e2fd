/* libsrganst.so - C ABI of the MI355X (gfx950) SRGAN-ST training hot path.
 *
 * The reference (SebastianBitsch/SRGAN-ST) has no FFI of its own: its boundary is the Python
 * module surface.  These entry points sit underneath that surface; each one cites
 * the reference code it replaces.  Conventions:
 *   - every function returns int: 0 = ok, <0 = error (message: sst_last_error(), thread-local);
 *   - all pointers are DEVICE pointers to fp32 unless stated; the caller owns every buffer
 *     (inputs, outputs, saved-for-backward, workspace) - the library never allocates;
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*), re-entrant,
 *     graph-capturable (no sync, no malloc inside);
 *   - `counter` words must be zero on first use; kernels leave them zero again.
 */
#ifndef SRGANST_H
#define SRGANST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* sst_last_error(void);
int sst_version(void);
const char* sst_arch(void);
/* forget the HIP runtime's sticky last error (left behind by e.g. a failed stream capture) before going on in eager mode;
 * returns the pending code (0 = none) */
int sst_clear_error(void);
/* dev switches (SST_* environment variables) are read once, at their first use; this forgets them (tests that toggle a switch) */
int sst_reload_env(void);

/* ---- structure-tensor loss: loss.py:380-413 + utils.py:194-280 (sigma=.5, rho=2 default) -------
 * sr, gt, dsr: NCHW [B,3,H,W].  gS: saved [B,3,H,W].  partials: sst_st_loss_workspace() floats.
 * fwd writes loss[0] = mean_b mean_px d  and gS = d(sum_px d)/d(Jxx,Jyy,Jxy)(sr).
 * bwd: dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * d loss / d sr.                        */
int sst_st_loss_workspace(int B, int H, int W, int64_t* partial_floats);
int sst_st_loss_fwd(const float* sr, const float* gt, float* loss, float* gS, float* partials,
                    unsigned* counter, int B, int H, int W, float sigma, float rho, int normalize,
                    void* stream);
int sst_st_loss_bwd(const float* sr, const float* gS, float* dsr, const float* scale_dev,
                    float scale_host, int accumulate, int B, int H, int W, float sigma, float rho,
                    void* stream);
/* ---- structure-tensor maps (analysis, no gradient): the fields the loss integrates, from the loss's own tile code -------
 * x, gt: NCHW [B,3,H,W]; gt may be null when only maps of x are asked for.  Every output is optional (null = not computed):
 *   Sx, Sgt   [B,3,H,W] (Jxx, Jyy, Jxy) of x / gt;   Fx, Fgt  [B,3,H,W] (t, c2, s2) with t = Jxx + Jyy,
 *   c2 = (Jxx - Jyy) / (t + 1e-12), s2 = 2 Jxy / (t + 1e-12);   d  [B,H,W] the per-pixel distance (the loss's integrand);
 *   tile_sums [B,tiles] fp32 sum of d over each 32x32 tile's valid pixels (tiles row-major; sst_st_maps_workspace() floats in all) -
 *   the caller sums them per image (fp64, index order) for a per-image distance.  Sgt, Fgt, d and tile_sums need gt.
 * Axis convention of the reference (utils.py:219): "x" is the HEIGHT axis - Jxx is the energy of row-to-row variation (c2 = +1).
 * One launch; no atomics, no counter, no allocation, no sync; bit-identical from call to call.                          */
int sst_st_maps_workspace(int B, int H, int W, int64_t* tile_floats);
int sst_st_maps(const float* x, const float* gt, float* Sx, float* Sgt, float* Fx, float* Fgt, float* d, float* tile_sums,
                int B, int H, int W, float sigma, float rho, int normalize, void* stream);
/* The same two launches with the pixel criterion of the step riding along (reference train.py:129-140 evaluates "Pixel" =
 * MSE / L1, config.py:88-90, and "ST" on the same sr / gt): pix_mode 0 = MSE, 1 = L1.
 * fwd: also pix_loss[0] = mean over all B*3*H*W elements (pix_partials: as many floats as `partials`).
 * bwd: dsr (+)= (scale_dev ? *scale_dev : 1) * (scale_host * d ST-loss / d sr + pix_weight * d pixel criterion / d sr).   */
int sst_st_pixel_loss_fwd(const float* sr, const float* gt, float* loss, float* gS, float* partials, unsigned* counter,
                          float* pix_loss, float* pix_partials, int pix_mode, int B, int H, int W, float sigma, float rho,
                          int normalize, void* stream);
int sst_st_pixel_loss_bwd(const float* sr, const float* gt, const float* gS, float* dsr, const float* scale_dev, float scale_host,
                          float pix_weight, int pix_mode, int accumulate, int B, int H, int W, float sigma, float rho,
                          void* stream);
/* ---- structure-tensor loss and maps at any (sigma, rho) with radii R1 <= 8, R2 <= 20 (csrc/st_general.hip):
 * separable 1-D passes over whole planes in a caller-provided workspace, radii as runtime values.  The entries above keep their
 * two tile builds and their refusals; these run every pair within the bound (the two built pairs included).
 * sst_st_route (host only): *r1, *r2 = the radii; returns 0 when (sigma, rho) selects a tile build, 1 for the general path, and
 *   SST_ERR_UNSUPPORTED "... (sigma,rho)=(..) -> radii (..) not built" when R1 > 8 or R2 > 20.
 * sst_st_general_workspace: floats, with N = B*H*W: scratch 14 N (one buffer for forward, backward and maps), saved 2 N (Ix, Iy of
 *   sr: the forward writes them, the backward reads them), partials B * ceil(H/32) * ceil(W/32).
 * fwd: loss[0], gS as sst_st_loss_fwd; counter must be 0 at the first call and re-arms itself.   bwd: as sst_st_loss_bwd, from
 *   `saved` in place of sr.   maps: sst_st_maps's outputs and layouts.  Everything is validated on the host before any launch.   */
int sst_st_route(float sigma, float rho, int* r1, int* r2);
int sst_st_general_workspace(int B, int H, int W, int64_t* scratch_floats, int64_t* saved_floats, int64_t* partial_floats);
int sst_st_general_fwd(const float* sr, const float* gt, float* loss, float* gS, float* saved, float* scratch, float* partials,
                       unsigned* counter, int B, int H, int W, float sigma, float rho, int normalize, void* stream);
int sst_st_general_bwd(const float* saved, const float* gS, float* dsr, float* scratch, const float* scale_dev, float scale_host,
                       int accumulate, int B, int H, int W, float sigma, float rho, void* stream);
int sst_st_general_maps(const float* x, const float* gt, float* Sx, float* Sgt, float* Fx, float* Fgt, float* d, float* tile_sums,
                        float* scratch, int B, int H, int W, float sigma, float rho, int normalize, void* stream);
/* ---- SSIM loss (loss.py: SSIMLoss; csrc/ssim_loss.hip): loss[0] = 1 - mean(S) over batch, planes and the
 * (H-10) x (W-10) valid region of the 11-tap sigma 1.5 window, C1 = k1^2, C2 = k2^2 (images on the 0..1 scale).  sr, gt, dsr: NCHW
 * fp32 [B,3,H,W], H, W >= 11.  planes: 1 = one luma plane (65.481 R + 128.553 G + 24.966 B + 16) / 255, 3 = the RGB planes.
 * sst_ssim_loss_workspace: map_floats = B * planes * (H-10) * (W-10) * 3 (the forward's saved maps dS/da, dS/dexx, dS/dexy, laid out
 *   [B*planes][3][H-10][W-10]); partial_floats = 2 * B * planes * ceil((H-10)/32) * ceil((W-10)/32): one fp64 partial per workgroup,
 *   so `partials` must be 8-byte aligned.
 * fwd: maps may be null (no gradient wanted: nothing is written there).  counter must be 0 at the first call and re-arms itself;
 *   the partials are summed in index order by the last-arriving workgroup: one launch, the same bits in every run.
 * bwd: dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * d loss / d sr from the maps of the forward of the same (sr, gt); gt
 *   is a constant.  One launch.
 * Everything is validated on the host before any launch (null pointer, H or W < 11, planes not 1 or 3, k1 or k2 <= 0: non-zero
 * return, message in sst_last_error); no allocation, no sync, asynchronous on `stream`. */
int sst_ssim_loss_workspace(int B, int H, int W, int planes, int64_t* map_floats, int64_t* partial_floats);
int sst_ssim_loss_fwd(const float* sr, const float* gt, float* loss, float* maps, float* partials, unsigned* counter, int B, int H,
                      int W, int planes, double k1, double k2, void* stream);
int sst_ssim_loss_bwd(const float* sr, const float* gt, const float* maps, float* dsr, const float* scale_dev, float scale_host,
                      int accumulate, int B, int H, int W, int planes, void* stream);
/* ---- focal frequency loss (loss.py: FocalFrequencyLoss; csrc/freq_loss.hip): per image and RGB plane, with
 * d = sr - gt and D its orthonormal 2-D DFT, e = |D|^2, w = sqrt(e)^alpha / max over the plane of sqrt(e)^alpha (NaN -> 0, clamped to
 * [0,1], a constant for the gradient): loss[0] = mean over batch, planes and the H x W frequencies of w e.  sr, gt, dsr: NCHW fp32
 * [B,3,H,W], 1 <= H, W <= 512 (any size: a direct DFT), B >= 1 and 3 B <= 65535; alpha finite and >= 0.  With Wh = W/2 + 1 (the half
 * spectrum kx = 0 .. W/2; column 0 counts once, column W/2 once when W is even, every other column twice) and S = B*3*H*Wh*2:
 * sst_freq_loss_workspace: saved_floats = S (w .* D as interleaved (re, im), laid out [B*3][H][Wh]: written by the forward, read by
 *   the backward, owned by the call); scratch_floats = 2 S + B*3 * ceil(Wh/32) * ceil(H/32) (the row-pass output [B*3][Wh][H] complex,
 *   the spectrum [B*3][H][Wh] complex, then one maximum of e per workgroup of the column pass; the backward reuses the first S floats;
 *   contents are dead between entries, so one buffer per criterion serves every call of a shape); partial_floats =
 *   2 * B*3 * ceil(H*Wh/1024): one fp64 partial per workgroup of the weighting kernel.  saved, scratch and partials must be 8-byte
 *   aligned; counter is one 32-bit word, 0 at the first call, and re-arms itself.
 * fwd: three launches (rows, columns, weighting); saved may be null (no gradient wanted: nothing is written there).  The partials are
 *   summed in index order by the last-arriving workgroup: the same bits in every run.
 * bwd: two launches (columns, rows): dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * d loss / d sr from `saved`; gt is a constant.
 * Everything is validated on the host before any launch (null pointer, B < 1, H or W outside 1..512 "... size HxW not built", alpha
 * negative or not finite, grid limits: non-zero return, message in sst_last_error); no allocation, no sync, asynchronous on `stream`. */
int sst_freq_loss_workspace(int B, int H, int W, int64_t* saved_floats, int64_t* scratch_floats, int64_t* partial_floats);
int sst_freq_loss_fwd(const float* sr, const float* gt, float* loss, float* saved, float* scratch, float* partials, unsigned* counter,
                      int B, int H, int W, double alpha, void* stream);
int sst_freq_loss_bwd(const float* saved, float* dsr, float* scratch, const float* scale_dev, float scale_host, int accumulate, int B,
                      int H, int W, void* stream);
/* ---- back-projection loss (loss.py: BackProjectionLoss, metrics.py: lr_consistency; csrc/bp_loss.hip): with
 * down(x)[oy][ox] = sum_tx wx[ox][tx] * (sum_ty wy[oy][ty] * x[iy[oy][ty]][ix[ox][tx]]) - sst_bicubic's arithmetic: fp32 FMAs, taps
 * in table order, the vertical sum inside - D = down(sr) - T and loss[0] = mean over B*3*oh*ow of |D| (criterion 0) or D^2
 * (criterion 1).  sr, gt, dsr: NCHW fp32 [B,3,H,W]; scale 2, 4 or 8; oh = H / scale, ow = W / scale; H, W >= scale, any values;
 * 1 <= B <= 21845.  wy / iy [oh,Ty], wx / ix [ow,Tx]: the tap tables of bicubic.py at 1 / scale in device memory (fp32 weights,
 * int32 0-based indices that grow with the output and the tap), 1 <= Ty, Tx <= 4 scale + 2.
 * sst_bp_loss_workspace: saved_floats = B*3*oh*ow (rho'(D) = sign(D), sign(0) = 0, or 2 D, laid out [B,3,oh,ow]: written by the
 *   forward, read by the backward, owned by the call); partial_floats = 2 * B*3 * ceil(oh/8) * ceil(ow/tile), tile = 32 LR columns
 *   (16 at scale 8): one fp64 partial per workgroup, so `partials` must be 8-byte aligned.
 * fwd: one launch.  Exactly one of gt and lr is non-null: gt [B,3,H,W] gives T = down(gt), rounded to the 1/255 grid
 *   (rintf(255 v) / 255: the bits of sst_bicubic(gt, round_grid = 1)) when round_target; lr [B,3,oh,ow] is T itself.  saved may be
 *   null (no gradient wanted: nothing is written there); per_image may be null, else fp64 [B]: the mean of rho(D) per image, from the
 *   same partials.  clamp_sr: sr is clamped to [0,1] as it is loaded (the metric; refused together with saved).  counter is one
 *   32-bit word, 0 at the first call, and re-arms itself; the partials are summed in index order by the last-arriving workgroup:
 *   the same bits in every run.
 * bwd: one launch, a gather: dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * down^T(saved) / (B*3*oh*ow) through the transposed
 *   tables ti_y / tw_y [H,Ny], ti_x / tw_x [W,Nx]: per input row (column) the (output index, weight) pairs of the outputs that read
 *   it (the taps of one output clamped onto a border pixel listed one by one or merged), packed to the front; a list ends at the
 *   first index < 0 (1 <= Ny, Nx <= 64).
 * Everything is validated on the host before any launch (null pointer, both or neither of gt / lr, saved with clamp_sr, scale,
 * criterion, B < 1, H or W < scale "image WxH is below ...", tap counts, list widths, grid limits: non-zero return, message in
 * sst_last_error); no allocation, no sync, asynchronous on `stream`. */
int sst_bp_loss_workspace(int B, int H, int W, int scale, int64_t* saved_floats, int64_t* partial_floats);
int sst_bp_loss_fwd(const float* sr, const float* gt, const float* lr, float* loss, double* per_image, float* saved, float* partials,
                    unsigned* counter, const float* wy, const int* iy, const float* wx, const int* ix, int B, int H, int W, int scale,
                    int Ty, int Tx, int criterion, int round_target, int clamp_sr, void* stream);
int sst_bp_loss_bwd(const float* saved, float* dsr, const float* tw_y, const int* ti_y, const float* tw_x, const int* ti_x,
                    const float* scale_dev, float scale_host, int accumulate, int B, int H, int W, int scale, int Ny, int Nx,
                    void* stream);
/* ---- gradient-magnitude and gradient-variance losses (loss.py: GradientLoss, GradientVarianceLoss; csrc/grad_loss.hip, DESIGN.md
 * section 19).  sr, gt, dsr: NCHW fp32 [B,3,H,W].  Gv, Gh: the zero-padded 3x3 correlations (F.conv2d, padding 1) with the vertical
 * operator - op 0 "central" [[0,-1,0],[0,0,0],[0,1,0]], op 1 "sobel" [[-1,-2,-1],[0,0,0],[1,2,1]] - and with its transpose.
 * Gradient loss, per image and RGB plane: M(I) = sqrt(Gv(I)^2 + Gh(I)^2 + eps); loss[0] = mean over B*3*H*W of |M(sr) - M(gt)|
 *   (crit 0) or of its square (crit 1).  Any H, W >= 1; 1 <= B <= 21845; eps finite and > 0.
 * sst_grad_loss_workspace: partial_floats = 2 * B*3 * ceil(H/32) * ceil(W/32): one fp64 partial per workgroup, so `partials` must be
 *   8-byte aligned.
 * fwd: one launch, nothing is saved.  counter is one 32-bit word, 0 at the first call, and re-arms itself; the partials are summed in
 *   index order by the last-arriving workgroup: the same bits in every run.
 * bwd: one launch, a gather (no atomics): dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * d loss / d sr, recomputed from sr and
 *   gt with the forward's op, crit and eps; gt is a constant; the derivative of |.| at a tie is 0.  scale_dev may be null.
 * Gradient-variance loss, on gray = 0.2989 R + 0.587 G + 0.114 B with the Sobel operator: the two response maps are cut into
 *   non-overlapping patch x patch blocks from the top-left corner, PH = H / patch by PW = W / patch of them (leftover rows and columns
 *   belong to no patch); v = the unbiased variance of a block; loss[0] = mean((vv(sr) - vv(gt))^2) + mean((vh(sr) - vh(gt))^2), each
 *   mean over B*PH*PW.  2 <= patch <= 32; H, W >= patch; 1 <= B <= 65535.
 * sst_gv_loss_workspace: saved_floats = 4 * B * PH * PW (per patch: mean of sr's Gv, d loss / d vv, mean of sr's Gh, d loss / d vh, laid
 *   out [B,PH,PW,4]: written by the forward, read by the backward, owned by the call); partial_floats = 2 * B * ceil(PH/n) * ceil(PW/n)
 *   with n = 32 / patch (integer division) patches per tile side: one fp64 partial per workgroup, `partials` 8-byte aligned.
 * fwd: one launch; saved may be null (no gradient wanted: nothing is written there); counter as above.
 * bwd: one launch, a gather: dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * d loss / d sr from sr and `saved` of the forward of
 *   the same sr; gt is not read.  Every pixel of dsr is written, leftover rows and columns included.  scale_dev may be null.
 * Everything is validated on the host before any launch (null pointer, B < 1, H or W < 1 or below patch, op or crit not 0 / 1, eps not
 * finite or <= 0, patch outside 2..32, grid limits: non-zero return, message in sst_last_error); no allocation, no sync, asynchronous
 * on `stream`. */
int sst_grad_loss_workspace(int B, int H, int W, int64_t* partial_floats);
int sst_grad_loss_fwd(const float* sr, const float* gt, float* loss, float* partials, unsigned* counter, int B, int H, int W, int op,
                      int crit, double eps, void* stream);
int sst_grad_loss_bwd(const float* sr, const float* gt, float* dsr, const float* scale_dev, float scale_host, int accumulate, int B,
                      int H, int W, int op, int crit, double eps, void* stream);
int sst_gv_loss_workspace(int B, int H, int W, int patch, int64_t* saved_floats, int64_t* partial_floats);
int sst_gv_loss_fwd(const float* sr, const float* gt, float* loss, float* saved, float* partials, unsigned* counter, int B, int H,
                    int W, int patch, void* stream);
int sst_gv_loss_bwd(const float* sr, const float* saved, float* dsr, const float* scale_dev, float scale_host, int accumulate, int B,
                    int H, int W, int patch, void* stream);
/* ---- artifact-map (LDL) loss (loss.py: ArtifactLoss; csrc/artifact_loss.hip).  sr, gt, ref, dsr: NCHW fp32
 * [B,3,H,W]; ref (the averaged generator's output) may be null.  ksize = k odd, 3..11, p = k / 2; H, W >= p + 1; 1 <= B <= 65535.
 *   r = |gt - sr| summed over R, G, B (r_e the same of ref); s_b = (unbiased variance of r over image b)^(1/5); v = the unbiased
 *   variance of the k x k window of r, reflect-padded by p; w = s_b v, and 0 where r < r_e; loss[0] = mean over B*3*H*W of w |sr - gt|.
 *   w is a constant of the gradient: d loss / d sr = w sign(sr - gt) / (3 B H W), sign(0) = 0.
 * sst_artifact_loss_workspace: with T = B * ceil(H/32) * ceil(W/32) workgroups, map_floats = B*H*W (w, one float per pixel: written by
 *   the forward, read by the backward, owned by the call), stat_floats = 2 * (2 T + B) (fp64: two sums per workgroup, then the B global
 *   weights), partial_floats = 2 * T (one fp64 partial per workgroup); `stats` and `partials` must be 8-byte aligned.
 * fwd: two launches (the per-image variance and s_b; the map and the loss).  wmap may be null (no gradient wanted: nothing is written
 *   there).  stat_counter and counter are one 32-bit word each, 0 at the first call, and re-arm themselves; every sum is taken in a
 *   fixed order by a last-arriving workgroup: no float atomics, the same bits in every run.
 * bwd: one launch: dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * w sign(sr - gt) / (3 B H W) from sr, gt and `wmap` of the
 *   forward of the same sr; every element of dsr is written.  scale_dev may be null.
 * Everything is validated on the host before any launch (null pointer, B < 1, ksize even or outside 3..11, H or W < p + 1, alignment,
 * grid limits: non-zero return, message in sst_last_error); no allocation, no sync, asynchronous on `stream`. */
int sst_artifact_loss_workspace(int B, int H, int W, int ksize, int64_t* map_floats, int64_t* stat_floats, int64_t* partial_floats);
int sst_artifact_loss_fwd(const float* sr, const float* gt, const float* ref, float* loss, float* wmap, float* stats,
                          unsigned* stat_counter, float* partials, unsigned* counter, int B, int H, int W, int ksize, void* stream);
int sst_artifact_loss_bwd(const float* sr, const float* gt, const float* wmap, float* dsr, const float* scale_dev, float scale_host,
                          int accumulate, int B, int H, int W, int ksize, void* stream);

/* ---- convolution (fp32 MFMA implicit GEMM, NHWC) --------------------------------------------------
 * Replaces the cuDNN/oneDNN kernels behind nn.Conv2d fwd/bwd of model.py:32-56,101,113,127,159,173,176.
 * Weights are consumed in a fragment-major packed layout produced by sst_conv_pack from the reference
 * layout [Cout][Cin][k][k]:  mode 0 = forward, mode 1 = data-gradient of a stride-1 conv (transposed,
 * rotated 180 deg; then outputs = Cin, inputs = Cout).
 * in_act: 0 none, 1 slope activation (PReLU scalar / LeakyReLU / ReLU=slope 0) applied to
 *         x*in_scale+in_shift while staging (the producer's BatchNorm-apply + activation, fused).
 * out_mode: 0 NHWC, 1 PixelShuffle(2) store (model.py:160), 2 NCHW + clamp(0,1) with pre-clamp copy
 *           (model.py:148-150), 3 inverse pixel-shuffle store.
 * stats: per-tile BatchNorm partials [sst_conv_stat_tiles][2][Cout] (sum, centred M2), stats_cnt [tiles].
 * The packed buffer of a 3x3 conv with 64 inputs and Cout % 16 == 0 carries a second copy of the weights in the layout
 * of the band kernel (csrc/conv_band.hip), which sst_conv_fwd / sst_conv_dgrad_* use for stride-1 NHWC stores when the
 * image rows group into bands of 144 or 48 pixels (the SRResNet trunk shape, model.py:173,176,113). */
int64_t sst_conv_packed_floats(int Cout, int Cin, int ksize);
int sst_conv_pack(const float* w, float* wp, int Cout, int Cin, int ksize, int mode, void* stream);
/* one launch for many tensors: jobs = device array of {const float* w; float* wp; int Cout, Cin, KK, mode;
 * long long total, block_begin;} (48 bytes each; each workgroup packs 1024 floats).  mode 0 / 1: sst_conv_pack forward /
 * data-gradient layout; 2 / 3: sst_conv9_c3_pack mode 0 / 1; 4: sst_conv9_to3_pack (total = the matching *_packed_floats) */
int sst_conv_pack_multi(const void* jobs, int njobs, int total_blocks, void* stream);
int sst_conv_mtiles(int B, int Ho, int Wo);
/* first dimension of stats / stats_cnt / epi_partial written by the NHWC-store conv of this shape (input H x W):
 * one tile per band when the band kernel takes the shape, else sst_conv_mtiles of the output size */
int sst_conv_stat_tiles(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
/* kernel the conv / weight-gradient entries dispatch to for a shape when called plain - no bias, input affine, activation,
 * statistics or residual - in rocprofv3 spelling without the argument list: labels for bench.py's roofline rows, to be matched
 * against profiles/.  Both report the launcher's own selection (conv_fwd_select / wgrad_plan), dev switches included. */
const char* sst_conv_kernel_name(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int out_mode, int fused_in);
const char* sst_conv_wgrad_kernel_name(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int njobs);
long sst_debug_big_tile_launches(void);   /* test hook: launches of the 64x64-tile conv kernel so far */
long sst_debug_band_launches(void);       /* test hook: launches of the band conv kernel so far */
long sst_debug_wgrad_band_launches(void); /* test hook: launches of the all-taps weight-gradient kernel so far */
/* measurement hook (tools/mfma_peak.py): `blocks` workgroups x 4 waves x iters x 4 v_mfma_f32_32x32x2_f32, no memory traffic */
int sst_debug_mfma_peak(float* out, int blocks, int iters, void* stream);
/* measurement hook (tools/bf16x3_probe.py): the split-operand bf16 MFMA form proposed in DESIGN.md section 8 - mode 0: one 32 x 32 x K
 * product by the fp32 MFMA (C32) and by six bf16 MFMAs per 16 k (C3) for an accuracy comparison on the host; mode 1: rate of the
 * six-MFMA group in a register-only loop (C32 = scratch, K = iterations, blocks workgroups).  Not used by the product path. */
int sst_debug_bf16x3(const float* A, const float* B, float* C32, float* C3, int K, int mode, int blocks, void* stream);
/* measurement hook (tools/stamp_step.py): out[slot] = the device's 100 MHz wall clock at the point of the stream / captured graph */
int sst_debug_stamp(unsigned long long* out, int slot, void* stream);
int sst_conv_fwd(const float* x, const float* wp, float* y, float* y_pre, const float* bias,
                 const float* in_scale, const float* in_shift, const float* in_slope,
                 float in_slope_const, int in_act, const float* residual, float* stats,
                 float* stats_cnt, int out_mode, int B, int H, int W, int Cin, int Cout, int ksize,
                 int stride, void* stream);
/* ---- persistent, software-pipelined form of the 3x3 conv (csrc/conv_pipe.hip) for the discriminator's layers
 * (model.py:30-59) and their stride-1 data-gradients: Cin % 64 == 0, Cout % 32 == 0, NHWC store, stride 1 / 2 (even H, W),
 * at least 256 tiles of 32 px x 32 ch.  The batch is tiled as one tall image (no MFMA lanes on padding pixels of the
 * 12 x 12 / 6 x 6 layers), the next input patch and the weight fragments are in flight while the MFMAs of the current
 * stage run, layers with few tiles split K over workgroups (partial slabs in `ws`, summed in fixed order).
 * sst_conv_pipe_supported: the tile width (8 / 4 / 2) when the shape is taken, else 0 (the 64 -> 64 trunk shape of the band kernel is never taken).  stats / stats_cnt / epi_partial have sst_conv_pipe_stat_tiles rows
 * (a different tiling than sst_conv_stat_tiles); ws = sst_conv_pipe_ws_floats floats (0: not needed).
 * Arguments as sst_conv_fwd (forward statistics) / sst_conv_dgrad_bwdstats (epi_*: backward partials). */
int sst_conv_pipe_supported(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
int sst_conv_pipe_stat_tiles(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
int64_t sst_conv_pipe_ws_floats(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
/* COEFFICIENT GROUPS: several passes of the network over different inputs with the same weights - the discriminator step's
 * D(gt) and D(sr.detach()), train.py:155-158 - run as ONE batch of B images in which every grp_images consecutive images form a
 * pass with its own train-mode BatchNorm statistics.  The per-channel arrays in_scale / in_shift / epi_scale / epi_shift are then
 * [B / grp_images][channels] (row = pass); stats / epi_partial tiles never straddle a pass (sst_conv_pipe_groups_ok: the pass
 * boundary falls on a tile boundary of the tall image), so the tile rows of pass p are the p-th of B / grp_images equal consecutive
 * ranges.  grp_images = 0 (or B): one row for the whole batch. */
int sst_conv_pipe_groups_ok(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int grp_images);
int sst_conv_pipe_fwd_grp(const float* x, const float* wp, float* y, const float* bias, const float* in_scale,
                          const float* in_shift, const float* in_slope, float in_slope_const, int in_act, float* stats,
                          float* stats_cnt, const float* epi_y, const float* epi_scale, const float* epi_shift,
                          const float* epi_slope, float epi_slope_const, int epi_act, float* epi_partial, float* ws, int B,
                          int H, int W, int Cin, int Cout, int ksize, int stride, int grp_images, void* stream);
/* "N-split" form of the pipelined kernel (csrc/conv_nsplit.hip) for Cout % 128 == 0 and at least 1024 (tile, 128-channel group) units
 * (512 with out_mode = 1, the PixelShuffle(2) store of sst_conv_fwd - model.py:160 - which the K-split kernel does not have; no
 * statistics / partials with it):
 * the 4 waves of a workgroup share one staged patch and each computes the full K for its own 32 output channels - no K-partial
 * exchange, a quarter of the patch traffic per MFMA.  Same arguments, packed weights and statistics tiling as sst_conv_pipe_fwd_grp
 * (no split-K workspace); sst_conv_ns_supported: tile width when the shape is taken, else 0. */
int sst_conv_ns_supported(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int out_mode);
int sst_conv_ns_fwd(const float* x, const float* wp, float* y, const float* bias, const float* in_scale,
                    const float* in_shift, const float* in_slope, float in_slope_const, int in_act, float* stats,
                    float* stats_cnt, const float* epi_y, const float* epi_scale, const float* epi_shift,
                    const float* epi_slope, float epi_slope_const, int epi_act, float* epi_partial, int B, int H, int W,
                    int Cin, int Cout, int ksize, int stride, int out_mode, int grp_images, void* stream);
/* stride-2 data-gradient (sst_conv_s2_dgrad below) on the pipelined kernel: the four parity classes of a block of class pixels in
 * one unit (they share the dY patch), the 9 (class, tap) pairs in the place of the 9 taps, one accumulator per class.  Even H, W;
 * Cout % 64 == 0, Cin % 32 == 0.  wp = the buffer of sst_conv_s2_dgrad_pack; ws = sst_conv_s2_dgrad_pipe_ws_floats floats (0: none).
 * sst_conv_s2_dgrad_pipe_supported: tile width when the shape is taken, else 0. */
int sst_conv_s2_dgrad_pipe_supported(int B, int H, int W, int Cin, int Cout);
int64_t sst_conv_s2_dgrad_pipe_ws_floats(int B, int H, int W, int Cin, int Cout);
/* The epilogue can write the BatchNorm / activation backward partials of dx against epi_y (the saved output of the layer below,
 * [B,H,W,Cin]): epi_partial [sst_conv_s2_dgrad_pipe_stat_tiles()][3][Cin], the layout sst_bwd_finalize consumes (null: none; the
 * epi_* arguments are then unused).  Coefficient groups (sst_conv_pipe_fwd_grp): epi_scale / epi_shift [B / grp_images][Cin]. */
int sst_conv_s2_dgrad_pipe_stat_tiles(int B, int H, int W, int Cin, int Cout);
int sst_conv_s2_dgrad_pipe_groups_ok(int B, int H, int W, int Cin, int Cout, int grp_images);
int sst_conv_s2_dgrad_pipe_bwdstats_grp(const float* dy, const float* wp, float* dx, float* ws, const float* epi_y,
                                    const float* epi_scale, const float* epi_shift, const float* epi_slope,
                                    float epi_slope_const, int epi_act, float* epi_partial, int B, int H, int W, int Cin,
                                    int Cout, int grp_images, void* stream);
/* stride-1 data-gradient (mode 1 weights) whose epilogue also emits the BatchNorm/activation BACKWARD partial sums of
 * its result g against the saved conv output epi_y: epi_partial [sst_conv_stat_tiles][3][Cout] = per-tile sums of
 * (gz, gz*epi_y, g*min(z,0)) - the layout sst_bwd_finalize consumes (replaces a separate sst_bwd_reduce_grp pass). */
int sst_conv_dgrad_bwdstats(const float* x, const float* wp, float* y, const float* residual, const float* epi_y,
                            const float* epi_scale, const float* epi_shift, const float* epi_slope,
                            float epi_slope_const, int epi_act, float* epi_partial, int B, int H, int W, int Cin,
                            int Cout, int ksize, void* stream);
/* ---- accumulator mode of the BatchNorm statistics (trunk shape only: sst_conv_acc_supported): the producer conv adds its
 * per-band (sum, Chan-form sum of squares) into fp64 accumulators acc[nrep][C][2] (zero before the launch) with hardware
 * atomics; the consumer conv derives batch statistics + affine of its input from them in its prologue and publishes
 * mean / rstd / scale / shift (+ running statistics) once.  Replaces sst_bn_finalize_grp launches of model.py:174-177's BatchNorms.
 * in2 == null: staged = act(x*scale+shift); in2 != null: staged = x + in2*scale + shift, also written to side_out. */
int sst_conv_acc_supported(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
int sst_conv_fwd_acc(const float* x, const float* in2, float* side_out, const float* ones, const float* wp, float* y,
                     const float* bias, const float* in_slope, float in_slope_const, int in_act, const double* in_acc,
                     const float* in_gamma, const float* in_beta, float in_n, float eps, float momentum, float* o_mean,
                     float* o_rstd, float* o_scale, float* o_shift, float* run_mean, float* run_var, double* st_acc,
                     int nrep, int B, int H, int W, int Cin, int Cout, int ksize, void* stream);
/* one BatchNorm-backward stage in accumulator mode: coefficients from bw_in_acc [nrep][64][4] + mean/rstd/gamma (prologue),
 * next stage's sums added into bw_st_acc [nrep][Cout][4] (epilogue); dgamma/dbeta/dslope written once.  Replaces the
 * sst_bwd_finalize launch between two sst_conv_dgrad_fused stages. */
int sst_conv_dgrad_fused_acc(const float* g, const float* y2, const float* in_scale, const float* in_shift,
                             const float* in_slope, float in_slope_const, int in_act, float* dy_out, const float* wp,
                             float* out, const float* residual, const float* epi_y, const float* epi_scale,
                             const float* epi_shift, const float* epi_slope, float epi_slope_const, int epi_act,
                             const double* bw_in_acc, const float* mean, const float* rstd, const float* gamma, float n,
                             float* dgamma, float* dbeta, float* dslope, double* bw_st_acc, int nrep, int B, int H,
                             int W, int Cin, int Cout, int ksize, void* stream);
int sst_bn_finalize_acc(const double* acc, int nrep, int C, float n, const float* gamma, const float* beta,
                        float* run_mean, float* run_var, float* mean, float* rstd, float* scale, float* shift,
                        float eps, float momentum, void* stream);
/* forward conv on a not-yet-materialised residual sum h = x + y2*bn_scale + bn_shift (model.py:180-186 -> next block's conv):
 * h is formed while the input tile is staged and also written to h_out; ones = [Cin] vector of 1.0f.  Replaces sst_bn_residual. */
int sst_conv_fwd_resin(const float* x, const float* y2, const float* ones, const float* bn_scale, const float* bn_shift,
                       float* h_out, const float* wp, float* y, const float* bias, float* stats, float* stats_cnt,
                       int B, int H, int W, int Cin, int Cout, int ksize, void* stream);
/* one launch per BatchNorm-backward stage: BN+activation backward apply on load (dy = cA*gz + cB*y2 + cC, also written
 * to dy_out for the weight-gradient kernel), data-gradient conv (+ residual), optional partials for the next stage. */
int sst_conv_dgrad_fused(const float* g, const float* y2, const float* cA, const float* cB, const float* cC,
                         const float* in_scale, const float* in_shift, const float* in_slope, float in_slope_const,
                         int in_act, float* dy_out, const float* wp, float* out, const float* residual,
                         const float* epi_y, const float* epi_scale, const float* epi_shift, const float* epi_slope,
                         float epi_slope_const, int epi_act, float* epi_partial, int B, int H, int W, int Cin, int Cout,
                         int ksize, void* stream);
/* dW[Cout][Cin][k][k] (+)= sum_pixels X'(shifted) * dY ; slab = sst_conv_wgrad_chunks2*k*k*Cout*Cin floats.
 * sst_conv_wgrad_chunks2: chunk count to size the slab of sst_conv_wgrad_grp (njobs = 1) / sst_conv_wgrad_grouped (njobs layers)
 * with; H, W = input size.
 * It is the launcher's own plan (wgrad_plan, csrc/conv_wgrad.hip): the chunks its kernel writes, or - where input affine, activation
 * or a dev switch decide between kernels of different chunk counts - the largest of them. */
int sst_conv_wgrad_chunks2(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int njobs);
/* in_scale / in_shift [B / grp_images][Cin]: the images are grp_images-sized passes with their own BatchNorm coefficients (see
 * sst_conv_pipe_fwd_grp), dW sums over all of them.  Taken by the all-taps tile kernel only (sst_conv_wgrad_groups_ok). */
int sst_conv_wgrad_groups_ok(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int grp_images);
int sst_conv_wgrad_grp(const float* x, const float* dy, float* slab, float* dw, const float* in_scale,
                   const float* in_shift, const float* in_slope, float in_slope_const, int in_act,
                   int B, int H, int W, int Cin, int Cout, int stride, int ksize, int accumulate,
                       int grp_images, void* stream);
/* Slab reduces of a whole backward pass in one launch: sst_conv_wgrad_grp with accumulate bit 2 (value 4) leaves its slab un-reduced
 * where sst_conv_wgrad_pending_reduce(...) > 0 (= the chunks the launcher's own plan writes for these arguments; 0: that launch writes dW itself and ignores the bit); the
 * caller then hands sst_wgrad_reduce_multi a HOST array of up to 24 jobs {const float* slab; float* dw; int nchunk, kk, Cout, Cin,
 * accumulate, reserved;} (40 bytes each).  Same arithmetic per job as the per-layer reduce (bit-identical dW). */
int sst_conv_wgrad_pending_reduce(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int has_in_scale, int in_act);
int sst_wgrad_reduce_multi(const void* jobs, int njobs, void* stream);
/* weight gradient of the two 9x9 convs with a 3-channel side (Generator.conv1 / conv3, model.py:101,127):
 * N = (kx, ch3) = 27 of 32 MFMA columns instead of 3.  kind 0 = conv3 (C->3), kind 1 = conv1 (3->C). */
int sst_wgrad_c3_supported(int C, int ksize);
int64_t sst_wgrad_c3_slab_floats(int B, int H, int W, int C);
int sst_wgrad_c3(const float* big, const float* small, float* slab, float* dw, const float* in_slope,
                 float in_slope_const, int in_act, int kind, int B, int H, int W, int C, int accumulate,
                 void* stream);

/* forward of the same two convs with the folding on the K side (conv1: 3->C, also conv3's data-gradient with
 * mode 1 weights) resp. the N side (conv3: C->3, stores NCHW + clamp like out_mode 2 of sst_conv_fwd). */
int64_t sst_conv9_c3_packed_floats(int Cout_eff);
int sst_conv9_c3_pack(const float* w, float* wp, int Cout, int Cin, int mode, void* stream);
int sst_conv9_c3_fwd(const float* x, const float* wp, float* y, const float* bias, int B, int H, int W,
                     int Cout, void* stream);
int64_t sst_conv9_to3_packed_floats(int C);
int sst_conv9_to3_pack(const float* w, float* wp, int C, void* stream);
int sst_conv9_to3_fwd(const float* x, const float* wp, float* y, float* y_pre, const float* bias,
                      const float* in_slope, float in_slope_const, int in_act, int B, int H, int W, int C,
                      void* stream);

/* data-gradient of a 3x3 / stride-2 / pad-1 conv (Discriminator.features model.py:35,42,49,56): the input-gradient
 * pixels are split into 4 parity classes, each a dense 1x1 / 1x2 / 2x1 / 2x2 correlation over dy. */
int64_t sst_conv_s2_dgrad_packed_floats(int Cout, int Cin);
int sst_conv_s2_dgrad_pack(const float* w, float* wp, int Cout, int Cin, void* stream);
int sst_conv_s2_dgrad(const float* dy, const float* wp, float* dx, int B, int H, int W, int Cin, int Cout,
                      void* stream);
/* one BatchNorm-backward stage around the stride-2 data-gradient (contract of sst_conv_dgrad_fused; g / y2 / dy_out live on the
 * conv's output side [B,Ho,Wo,Cout], dx / epi_y are [B,H,W,Cin]); epi_partial [sst_conv_s2_dgrad_tiles(B,H,W)][3][Cin] */
int sst_conv_s2_dgrad_tiles(int B, int H, int W);
/* kernel the two entries above launch for this shape, as rocprofv3 prints it (profiling labels): the launcher's own selection.
 * Where the four parity classes go out one launch each, it is the kernel of the class-0 launch. */
const char* sst_conv_s2_dgrad_kernel_name(int B, int H, int W, int Cin, int Cout, int fused);
int sst_conv_s2_dgrad_fused(const float* g, const float* y2, const float* cA, const float* cB, const float* cC,
                            const float* in_scale, const float* in_shift, const float* in_slope, float in_slope_const,
                            int in_act, float* dy_out, const float* wp, float* dx, const float* epi_y,
                            const float* epi_scale, const float* epi_shift, const float* epi_slope, float epi_slope_const,
                            int epi_act, float* epi_partial, int B, int H, int W, int Cin, int Cout, void* stream);

/* weight gradients of njobs <= 40 layers of IDENTICAL shape in ONE launch (the 33 trunk-shaped convs of the generator):
 * jobs = HOST array of {const float* x, *dy; float* slab, *dw; const float* in_scale, *in_shift, *in_slope;
 * float in_slope_const; int in_act;} (64 bytes each, device pointers inside); the table is handed to the kernels as a
 * by-value argument, so the call is graph-capturable without any device-side table. */
int sst_conv_wgrad_grouped(const void* jobs, int njobs, int B, int H, int W, int Cin, int Cout, int stride,
                           int ksize, int accumulate, void* stream);

/* ---- BatchNorm (train mode) + elementwise glue, tensors viewed as [R rows, C channels] -----------
 * nn.BatchNorm2d model.py:36-57,114,174,177 (eps 1e-5, momentum .1); PReLU/LeakyReLU backward;
 * residual adds model.py:146,183. */
/* `groups` passes batched as one tall image (see sst_conv_pipe_fwd_grp): stats / cnt hold ntiles tiles = groups equal consecutive
 * ranges; mean / rstd / scale / shift are [groups][C]; the running statistics take one momentum step per group, in group order. */
int sst_bn_finalize_grp(const float* stats, const float* cnt, int ntiles, int C, int groups, const float* gamma,
                        const float* beta, float* run_mean, float* run_var, float* mean, float* rstd, float* scale,
                        float* shift, float eps, float momentum, void* stream);
int sst_bn_eval_affine(const float* gamma, const float* beta, const float* run_mean,
                       const float* run_var, float* scale, float* shift, int C, float eps, void* stream);
int sst_bn_residual(const float* y, const float* scale, const float* shift, const float* res,
                    const float* res_slope, float* out, int64_t R, int C, void* stream);
int sst_bwd_reduce_blocks(int64_t R, int C);
int sst_bwd_finalize(const float* partial, int nblk, int C, float n, const float* mean,
                     const float* rstd, const float* gamma, float* dgamma, float* dbeta, float* cA,
                     float* cB, float* cC, float* dslope, int accumulate, void* stream);
/* the three backward steps for `groups` passes batched as one tensor of groups * R rows (R rows per pass): scale / shift / mean / rstd /
 * cA / cB / cC are [groups][C], partial is [groups][sst_bwd_reduce_blocks(R, C)][3][C], n = elements of ONE pass per channel;
 * dgamma / dbeta (the passes share the parameters) sum over the passes in group order. */
int sst_bwd_reduce_grp(const float* g, const float* g2, const float* y, const float* scale, const float* shift,
                       const float* slope, float slope_const, int act, float* partial, int64_t R, int C, int groups,
                       void* stream);
int sst_bwd_finalize_grp(const float* partial, int nblk, int C, float n, int groups, const float* mean, const float* rstd,
                         const float* gamma, float* dgamma, float* dbeta, float* cA, float* cB, float* cC, int accumulate,
                         void* stream);
int sst_bwd_apply_grp(const float* g, const float* g2, const float* y, const float* scale, const float* shift,
                      const float* slope, float slope_const, int act, const float* cA, const float* cB, const float* cC,
                      float* dy, int64_t R, int C, int groups, void* stream);
/* channel-parallel also with dslope (scratch: (C+63)/64 floats, counter: one zeroed word, left zero) */
int sst_bwd_finalize_wide(const float* partial, int nblk, int C, float n, const float* mean, const float* rstd,
                          const float* gamma, float* dgamma, float* dbeta, float* cA, float* cB, float* cC,
                          float* dslope, int accumulate, float* scratch, unsigned* counter, void* stream);
/* activation-only backward (PReLU / LeakyReLU, no BatchNorm) fused with the partial sums of the bias and slope
 * gradients: dy = act'(y)*(g+g2), optionally stored pre-PixelShuffle; partial [sst_act_bwd_partial_blocks][3][C or 4C]
 * in sst_bwd_finalize's layout (replaces reduce + finalize + apply + reduce + finalize of model.py:159-161's backward) */
int sst_act_bwd_partial_blocks(int64_t stored_rows);
int sst_act_bwd_partial(const float* g, const float* g2, const float* y, const float* slope, float slope_const,
                        float* dy, float* partial, int64_t R, int C, int unshuffle_H, int unshuffle_W, void* stream);
int sst_bwd_apply(const float* g, const float* g2, const float* y, const float* scale,
                  const float* shift, const float* slope, float slope_const, int act, const float* cA,
                  const float* cB, const float* cC, float* dy, int64_t R, int C, int unshuffle_H,
                  int unshuffle_W, void* stream);
int sst_add(const float* a, const float* b, float* out, int64_t n, void* stream);

/* ---- layout + criterions ------------------------------------------------------------------------
 * sst_transpose: NCHW <-> NHWC (model.py:138-152 keeps an NCHW surface).  sst_clamp_bwd: backward of
 * clamp_(0,1) model.py:150 fused with the NCHW->NHWC hand-off and the conv3 bias gradient.
 * pixel criterion config.py:88-90 (mode 0 MSE / 1 L1); BCEWithLogits config.py:71-73, train.py:113-161. */
int sst_transpose(const float* src, float* dst, int B, int C, int H, int W, int to_nchw, void* stream);
/* feature criterion on activated, per-channel-affine taps (ContentLossDiscriminator loss.py:231-289: BatchNorm(eval) + LeakyReLU
 * outputs of the discriminator): f(v) = act(v*scale[c]+shift[c]) with slope activation, loss = mean crit(f(x) - f(gt)) over a
 * [rows, C] tensor (mode 0 MSE, 1 L1); bwd: dx (+)= scale_host * scale_dev * dloss/dx */
int sst_feat_loss_fwd(const float* x, const float* gt, const float* scale, const float* shift, float slope, int C,
                      float* loss, float* partials, unsigned* counter, int64_t n, int mode, void* stream);
int sst_feat_loss_bwd(const float* x, const float* gt, const float* scale, const float* shift, float slope, int C,
                      float* dx, const float* scale_dev, float scale_host, int accumulate, int64_t n, int mode,
                      void* stream);
/* VGG19 feature stack pieces of ContentLossVGG (loss.py:11-70): ImageNet normalise fused with the layout change,
 * ReLU+MaxPool2d(2) forward/backward; the feature criterion is sst_pixel_loss_* with mode |= 2 (criterion on relu(x)). */
int sst_transpose_affine(const float* src, float* dst, int B, int C, int H, int W, int to_nchw,
                         const float* scale, const float* shift, void* stream);
int sst_maxpool_relu_fwd(const float* y, float* out, int B, int H, int W, int C, void* stream);
int sst_maxpool_relu_bwd(const float* g, const float* y, float* dy, int B, int H, int W, int C, void* stream);
int sst_clamp_bwd_blocks(int B, int H, int W);
int sst_clamp_bwd(const float* g, const float* pre, float* out, float* partial, float* dbias,
                  int accumulate, int B, int C, int H, int W, void* stream);
int sst_pixel_loss_blocks(int64_t n);
int sst_pixel_loss_fwd(const float* x, const float* gt, float* loss, float* partials, unsigned* counter,
                       int64_t n, int mode, void* stream);
int sst_pixel_loss_bwd(const float* x, const float* gt, float* dx, const float* scale_dev,
                       float scale_host, int accumulate, int64_t n, int mode, void* stream);
int sst_bce_logits(const float* logits, float target, float* loss, float* dlogits,
                   const float* scale_dev, float scale_host, int n, void* stream);
/* MATLAB-style antialiased bicubic resampling of bicubic.py:15-105 (LR synthesis of dataset.py:28) with host-built tap
 * tables: x [planes,H,W] -> y [planes,oh,ow]; wy/iy [oh,Ty], wx/ix [ow,Tx]; round_grid: round to the 1/255 grid (no clamp) */
int sst_bicubic(const float* x, float* y, const float* wy, const int* iy, const float* wx, const int* ix,
                int64_t planes, int H, int W, int oh, int ow, int Ty, int Tx, int round_grid, void* stream);
/* Training-batch gather from a device-resident uint8 crop store (device_data.py): src [N,H,W,3] HWC/RGB uint8, idx [B] int32
 * crop indices (device; repeats allowed; an index outside [0, N) yields NaN); lut [256] = float(u) / 255 (host-made);
 * gt [B,3,H,W] = lut[src[idx[b],y,x,c]] (may be null); lr [B,3,oh,ow] = the sst_bicubic of gt with round_grid, same tap tables
 * wy/iy [oh,Ty], wx/ix [ow,Tx] and same arithmetic (may be null).  One launch; no allocation, no sync (capturable). */
int sst_gather_batch(const uint8_t* src, int64_t N, const int* idx, int B, int H, int W, const float* lut, float* gt, float* lr,
                     const float* wy, const int* iy, const float* wx, const int* ix, int oh, int ow, int Ty, int Tx,
                     void* stream);
/* Training-batch gather from device-resident WHOLE images (device_data.py: DeviceImageArena): arena = packed HWC/RGB uint8 images
 * (base and arena_bytes multiples of 16); table [N,3] int64 = (byte offset, H_img, W_img) per image; desc [B,4] int32 (device,
 * 16-byte aligned) = (image, y0, x0, t) per sample.  With C = img[y0:y0+S, x0:x0+S] and t = 4*transpose + 2*vflip + 1*hflip, applied
 * in that order: out[y][x] = C[sy][sx], y' = t&2 ? S-1-y : y, x' = t&1 ? S-1-x : x, (sy,sx) = t&4 ? (x',y') : (y',x').
 * gt [B,3,S,S] = lut[out] (may be null); lr [B,3,oh,ow] = the sst_bicubic of gt with round_grid, tap tables of an S x S input (may be
 * null).  S % 4 == 0.  span: an upper bound of the number of consecutive crop rows one band needs (its LR row's taps and, with gt,
 * its own rows; sizes the LDS).  A descriptor out of range (image, window, t) yields NaN for that sample and reads nothing outside
 * the arena.  One launch; no allocation, no sync (capturable). */
int sst_gather_crops(const uint8_t* arena, int64_t arena_bytes, const int64_t* table, int64_t N, const int* desc, int B, int S,
                     const float* lut, float* gt, float* lr, const float* wy, const int* iy, const float* wx, const int* ix,
                     int oh, int ow, int Ty, int Tx, int span, void* stream);
/* ---- the blind-SR degradation stage (device_data.py: Degradation / degrade; csrc/degrade.h):
 *   lr = quantise( clamp( bicubic_down( x (*) k ) + n ) )   per sample, from its row of deg.
 * deg: int32 [B,8] (device, 32-byte aligned): the fp32 bit patterns of qa, qb, qc, sigma_n, then the Philox key k0, k1, then two zero
 * words.  Blur (skipped when qa < 0): w[dy][dx] = expf(-(qa dx^2 + qb dx dy + qc dy^2)) over the K x K window (K odd, 3..21, one
 * per launch), normalised by its fp64 sum, applied with torch's `reflect` padding as one fp32 FMA chain in row-major order.
 * Downscale: the bicubic of sst_gather_crops, term for term.  Noise (skipped when sigma_n == 0): sigma_n * z, z from Philox4x32-10
 * with counter (e, 0, 0, 0), e the element's index in the sample's [3,oh,ow] LR, and Box-Muller on its first two words.  A sample
 * with blur or noise is clamped to [0, 1]; one with neither takes sst_gather_crops' path and bits.  quantise = 0 writes the
 * unclamped, unrounded value (tests and tools).  Weights that do not sum to a finite positive number yield a NaN LR.
 * sst_gather_crops_degraded: sst_gather_crops (same arguments, lr not optional; span: with gt or without) with the stage between
 * the conversion and the LR; gt is what sst_gather_crops writes.  K / 2 < S.  One launch, no allocation, no sync (capturable).
 * sst_degrade: the same stage on x fp32 [B,3,H,W] -> lr [B,3,oh,ow], any H, W with K / 2 < min(H, W), through the same device code:
 * sst_gather_crops_degraded's lr equals sst_degrade of its gt bit for bit.  Tiled in rows and in columns of
 * sst_degrade_tile_cols() LR pixels.  One launch, no allocation, no sync. */
int sst_gather_crops_degraded(const uint8_t* arena, int64_t arena_bytes, const int64_t* table, int64_t N, const int* desc, int B,
                              int S, const float* lut, float* gt, float* lr, const float* wy, const int* iy, const float* wx,
                              const int* ix, int oh, int ow, int Ty, int Tx, int span, const int* deg, int K, int quantise,
                              void* stream);
int sst_degrade(const float* x, const int* deg, int B, int H, int W, int K, int quantise, float* lr, const float* wy, const int* iy,
                const float* wx, const int* ix, int oh, int ow, int Ty, int Tx, void* stream);
int sst_degrade_tile_cols(void);
/* ---- the JPEG stage of the degradation (device_data.py: jpeg / degrade(jpeg_chroma=...); csrc/jpeg.hip): a
 * baseline JPEG round trip in int32 arithmetic at every step, in place on lr fp32 [B,3,h,w] (h, w in 1..8192), after the stage above
 * has put it on the 1/255 grid.  Per sample Q = word 6 of its deg row (deg as above): 0 keeps the sample's bits, a Q outside 0..100
 * makes the sample NaN, else p = (int)rintf(255 clamp01(v)), 16-bit fixed-point YCbCr, MCUs of 8 x 8 (chroma = 0: 444) or 16 x 16
 * (chroma = 1: 420, chroma averaged 2 x 2 with rounding and replicated 2 x 2 on the way back) with edge replication, the Annex K
 * tables under libjpeg's quality rule, an 8-point DCT with T = rint(8192 C) and fixed shifts, n = sign(F) ((|F| + q 32768) / (q 65536)),
 * the inverse, 16-bit fixed-point RGB, out = (float)p / 255.f.  An MCU that holds a non-finite element comes out NaN in all three
 * channels.  The result does not depend on the batch position or on how the image is cut into workgroups.  One launch, no
 * allocation, no sync (capturable).
 * sst_jpeg_tables: the luminance then the chrominance table of a quality in 1..100, row-major, into out128 (host memory). */
int sst_jpeg(float* lr, const int* deg, int B, int h, int w, int chroma, void* stream);
int sst_jpeg_tables(int quality, int* out128);
/* ---- the second-order degradation stage (device_data.py: filter2d / SecondOrder; csrc/filter.hip): a K x K
 * correlation with a per-sample kernel taken from a table, then noise, clamp and the 1/255 grid, out of place: x, y fp32 [B,3,h,w]
 * (h, w in 1..8192; y == x is refused).  bank fp32 [M,K,K], row-major [dy][dx], 16-byte aligned, normalised by the host (the kernel
 * does not renormalise); K odd, 3..21, p = K / 2 < min(h, w) when M > 0; M == 0 with a null bank is legal (noise only).  flt int32
 * [B,8] (device, 32-byte aligned), per sample: the kernel index (-1: no blur), the fp32 bits of sigma_n, the fp32 bits of the shot
 * coefficient s_p, the gray flag (0 / 1), the Philox key k0, k1, two zero words.  Per sample:
 *   pass-through  idx == -1 && sigma_n == 0 && s_p == 0: y = the bits of x (NaNs and values outside [0, 1] included)
 *   blur   (idx >= 0)  v[y][x] = sum_{dy,dx} bank[idx][dy][dx] * X[refl(y+dy-p)][refl(x+dx-p)] - a correlation (F.conv2d's
 *          orientation), torch's `reflect` padding, one fp32 fmaf chain per pixel in row-major order from 0.f
 *   noise  (sigma_n != 0 || s_p != 0)  z from Philox4x32-10, counter (e, 0, 0, 0), Box-Muller as in the stage above; e the element's
 *          index in the sample's [3,h,w], or y*w + x with the gray flag (the three channels then get the same z);
 *          sd = s_p == 0 ? sigma_n : sqrtf(fmaf(s_p, fmaxf(v, 0), sigma_n^2));  v = fmaf(sd, z, v).  s_p is a heteroscedastic
 *          Gaussian (variance proportional to intensity: the Poisson-Gaussian model), not a Poisson sampler
 *   output clamp to [0, 1] by comparisons (a NaN is kept), then rintf(255 v) / 255.f; quantise = 0 writes the unclamped, unrounded v
 * An idx outside [-1, M), a gray flag outside {0, 1}, !(sigma_n >= 0) or !(s_p >= 0) makes that sample NaN and touches no other.  No
 * atomics: a result is a function of its sample's inputs alone, whatever the batch position, batch size and tile geometry.  One
 * launch, no allocation, no sync (capturable). */
int sst_filter2d(const float* x, float* y, const int* flt, const float* bank, int M, int B, int h, int w, int K, int quantise,
                 void* stream);
/* ---- the random resize round trip of the second-order stage (device_data.py: rescale / SecondOrder(resize_prob=...);
 * csrc/resize.hip): per sample, resample to an intermediate size (hi, wi), add noise there, resample back to
 * (h, w), clamp and the 1/255 grid, out of place: x, y fp32 [B,3,h,w] (h, w in 1..8192; y == x is refused).  rows int32 [B,8]
 * (device, 32-byte aligned), per sample: hi, wi (0, 0: no resize), the fp32 bits of sigma_n, the fp32 bits of the shot coefficient
 * s_p, the Philox key k0, k1, m1 | m2 << 2 | gray << 4 (m1: the mode of the resize to (hi, wi), m2: of the resize back; 0 area,
 * 1 bilinear, 2 bicubic), a zero word.  Per sample:
 *   pass-through  hi == wi == 0 && sigma_n == 0 && s_p == 0: y = the bits of x
 *   one axis n_in -> n_out, output index i, in integer arithmetic:  area: taps a = i n_in / n_out up to b = ((i + 1) n_in + n_out - 1)
 *          / n_out (exclusive), each 1 / (b - a).  num = (2i + 1) n_in - n_out, den = 2 n_out, f = floor(num / den), t = float(num -
 *          f den) / float(den);  bilinear (align_corners = False, no antialias): num < 0 gives f = t = 0, taps min(f, n_in - 1),
 *          min(f + 1, n_in - 1) with 1 - t, t;  bicubic (A = -0.75): taps clamp(f - 1 .. f + 2, 0, n_in - 1) with torch's cubic
 *          convolution coefficients of t.  At n_out == n_in every mode is the identity
 *   u      u[Y][X] = sum_j wy[j] (sum_i wx[i] x[iy_j][ix_i]), each sum one fp32 fmaf chain from 0.f in tap order (0, 0: u = x)
 *   noise  (sigma_n != 0 || s_p != 0)  sst_filter2d's rule on u, e = c hi wi + Y wi + X, or Y wi + X with the gray flag (0, 0: h, w
 *          stand in for hi, wi); the intermediate is neither clamped nor rounded
 *   back   (hi, wi) -> (h, w) with m2 by the same rule on u; then clamp and quantise as sst_filter2d does (quantise = 0: the raw value)
 * Exactly one of hi, wi zero, a negative one, 4 hi < h, hi > 2 h (the same for wi against w), a mode 3, a bit above bit 4 of word 6,
 * !(sigma_n >= 0) or !(s_p >= 0) makes that sample NaN and touches no other.  No atomics: a result is a function of its sample's
 * inputs alone, whatever the batch position, batch size and tile geometry.  One launch, no allocation, no sync (capturable). */
int sst_rescale(const float* x, float* y, const int* rows, int B, int h, int w, int quantise, void* stream);
/* ---- the random resize of the FIRST degradation stage (device_data.py: blur / rescale_to / Degradation(resize_prob=...);
 * csrc/resize.hip, csrc/degrade.hip).
 * sst_rescale_to: sst_rescale's chain with an output geometry of its own, out of place: x fp32 [B,3,H,W] -> y fp32 [B,3,h,w], H, W,
 * h, w in 1..8192, h <= H <= 16 h and w <= W <= 16 w (y == x is refused).  rows int32 [B,8] in sst_rescale's format.  Per sample:
 * resample (H, W) -> (hi, wi) with m1 by the one-axis rule above, the noise there (e = c hi wi + Y wi + X), neither clamp nor
 * rounding, resample (hi, wi) -> (h, w) with m2, then clamp and quantise (quantise = 0: the raw value).  hi == wi == 0 ("keep"): the
 * intermediate is the input itself, hi, wi = H, W, the noise at (H, W), then m2.  There is no pass-through when (H, W) != (h, w); at
 * (H, W) == (h, w) every row that sst_rescale accepts gives sst_rescale's bits.  Exactly one of hi, wi zero, a negative one, 8 hi < H,
 * hi > 2 H (the same for wi against W), a mode 3, a bit above bit 4 of word 6, !(sigma_n >= 0) or !(s_p >= 0) makes that sample NaN
 * and touches no other.  An area entry keeps its full tap count (H -> hi up to 9, hi -> h up to 2 H / h + 1).  No atomics: the same
 * bits whatever the batch position, batch size and tile geometry (SST_RESIZE1_TILE=RxC, a dev switch, fixes the output tile).  One
 * launch, no allocation, no sync (capturable).
 * sst_blur: the first stage's blur alone, out of place: y fp32 [B,3,H,W] = x (*) k per sample, unquantised, by sst_degrade's rule and
 * device code (deg rows as above; the noise word is not read): a sample's y is the image sst_degrade makes before its bicubic.  qa < 0
 * keeps the sample's bits.  K odd, 3..21, K / 2 < min(H, W).  One launch, no allocation, no sync (capturable). */
int sst_rescale_to(const float* x, float* y, const int* rows, int B, int H, int W, int h, int w, int quantise, void* stream);
int sst_blur(const float* x, const int* deg, float* y, int B, int H, int W, int K, void* stream);
/* Validation metrics of validate.image_metrics on the device (metrics.py), rounding for rounding: sr, hr fp32 NCHW [B,3,H,W] RGB;
 * out fp64 [B,2] = (MSE of the Y channel on the 0..255 scale over all H*W pixels, mean of the SSIM map over its (H-10) x (W-10)
 * valid region); sr_u8 / hr_u8: uint8 [B,H,W,3] BGR = tensor2img of each image (either may be null).  workspace:
 * sst_image_metrics_workspace() doubles.  H, W >= 11.  A NaN anywhere in sr or hr makes that image's two outputs NaN; its uint8
 * pixel is 0.  Two launches, partials summed in index order (bit-identical from run to run); no allocation, no sync. */
int sst_image_metrics_workspace(int B, int H, int W, int64_t* partial_doubles);
int sst_image_metrics(const float* sr, const float* hr, int B, int H, int W, double* out, uint8_t* sr_u8, uint8_t* hr_u8,
                      double* workspace, void* stream);
/* ---- tiled whole-image inference (upscale.py: Upscaler; csrc/tiles.hip).  t = 4*transpose + 2*vflip + 1*hflip as in
 * sst_gather_crops; all offsets 64-bit; one launch each, no allocation, no sync.
 * sst_tile_gather: one LR image [H,W] -> out fp32 [B,3,th',tw'] = the th x tw windows at (y0, x0) of desc [B,3] int32 (device) =
 * (y0, x0, t), each transformed by dihedral(t); (th',tw') = (tw,th) when t&4.  One t per call: a row whose t differs, or whose window
 * leaves the image, yields NaN for that tile and reads nothing.  Source, exactly one non-null: src_u8 HWC/RGB uint8 through lut [256]
 * = float(u) / 255 (bit-identical to u8.float() / 255; base 16-byte aligned, src_bytes a multiple of 16 that covers the image: the
 * buffer is padded) or src_f32 CHW fp32, copied (src_bytes >= 12*H*W). */
int sst_tile_gather(const uint8_t* src_u8, const float* src_f32, int64_t src_bytes, int H, int W, const int* desc, int B, int th,
                    int tw, int t, const float* lut, float* out, void* stream);
/* sst_tile_scatter: tiles fp32 [B,3,scale*th',scale*tw'] (the generator's output for the tiles of one sst_tile_gather call with the
 * same t) -> canvas fp32 [3,scale*H,scale*W].  rows [B,6] int32 (device) = (y0, x0, oy0, oy1, ox0, ox1) in LR pixels: of tile b,
 * mapped back through the inverse of t, the rectangle [oy0,oy1) x [ox0,ox1) of the image that it OWNS (inside its window) is stored
 * to the canvas, or added when accumulate != 0.  The owned rectangles of one call must be disjoint (no atomics); calls are ordered
 * by the stream.  Pixels that no row owns are not touched; a row outside the image or its window is skipped. */
int sst_tile_scatter(const float* tiles, const int* rows, int B, int H, int W, int th, int tw, int scale, int t, float* canvas,
                     int accumulate, void* stream);
/* sst_canvas_to_u8: canvas fp32 [3,H,W] -> out uint8 [H,W,3] RGB (4-byte aligned), q = rint(clamp(v * scale, 0, 1) * 255.f), NaN -> 0:
 * utils.tensor2img's arithmetic (sst_image_metrics's quantiser), channels left in RGB order.  scale: 1, or 0.125 for the sum of the
 * eight passes of the self-ensemble. */
int sst_canvas_to_u8(const float* canvas, int H, int W, float scale, uint8_t* out, void* stream);
/* ---- best-buddy losses (loss.py:78-142 BestBuddyLoss, loss.py:145-228 GramLoss, loss.py:292-375
 * PatchwiseStructureTensorLoss; ksize 3, stride 3, pad 0, squared-L2 matching):
 * sst_bb_patches cuts an image [B,3,H,W] into 27-vectors (unfold order) + squared norms inside the candidate table
 * cand [B,ncand,27] / cnrm [B,ncand]; sst_bb_match_dist pairs every SR patch with its best candidate (first minimum of
 * alpha*d(sr_i,c_j) + beta*d(gt_i,c_j), d = clamped expanded squared distance of utils.py:173-187) and produces the selected
 * indices, d(loss)/d(sr) and per-workgroup partial sums of the L1 / L2 criterion (loss = sum of partials) */
int sst_bb_blocks(int B, int H, int W);
/* feature mode: 0 raw patch (27, BestBuddyLoss), 1 gram matrix of the patch (9, GramLoss loss.py:145-228), 2 normalised
 * structure tensor of the 3x3 gray patch (27, PatchwiseStructureTensorLoss loss.py:292-375; st_mats = device [Ax 81][Ay 81][K 81],
 * the three 9x9 maps of utils.py:212-233 restricted to a zero-padded 3x3 image) */
int sst_bb_feature_dim(int mode);
int sst_bb_patches(const float* img, float* cand, float* cnrm, int B, int H, int W, int ncand_total, int cand_off,
                   int mode, const float* st_mats, void* stream);
/* the matching distance of utils.py:157-191 selectable (dist_l1 = 1: sum |x - y|; 0: the clamped expanded squared L2) */
int sst_bb_match_dist(const float* sr, const float* cand, const float* cnrm, int* ind, float* dsr, float* partials, int B,
                 int H, int W, int ncand, float alpha, float beta, int criterion_l2, int mode, const float* st_mats, int dist_l1,
                      void* stream);
/* General patch geometry for BestBuddyLoss (loss.py:86,116-129: F.unfold with any ksize <= 6, pad, stride; dist_norm 'l1' / 'l2'):
 * features in global tables [B, rows, D = 3 k k] (unfold order, zero padding).  sst_bbg_patches = F.unfold's patch count;
 * sst_bbg_unfold fills rows [row_off, row_off + patches) (+ squared norms or null); sst_bbg_match pairs the SR rows srf [B, np, D]
 * with the candidate table (first np rows = full-resolution GT patches): ind [B, np], gfeat [B, np, D] = d(loss)/d(SR patch entries),
 * partials [sst_bbg_blocks(B, np)] (loss = their sum); sst_bbg_fold = the unfold's adjoint, d(sr) [B,3,H,W] (overlapping patches summed
 * in fixed order). */
int sst_bbg_patches(int H, int W, int k, int pad, int stride);
int sst_bbg_blocks(int B, int np);
int sst_bbg_unfold(const float* img, float* table, float* nrm, int B, int H, int W, int k, int pad, int stride, int nrows_total,
                   int row_off, void* stream);
int sst_bbg_match(const float* srf, const float* cand, const float* cnrm, int* ind, float* gfeat, float* partials, int B, int np,
                  int ncand, int D, float alpha, float beta, int criterion_l2, int dist_l1, void* stream);
int sst_bbg_fold(const float* gfeat, float* dsr, int B, int H, int W, int k, int pad, int stride, void* stream);
int sst_weighted_sum(const float* const* terms, const float* weights, int n, float* out, float* weighted,
                     void* stream);

/* ---- discriminator classifier: flatten + Linear + LeakyReLU + Linear (model.py:61-65,69-70) -------
 * weights in the reference layout [N][K]; x [M][K], y [M][N], M <= 64.
 * sst_linear_dgrad: nhwc_HW > 0 scatters dx from the NCHW-flatten index k=(c,hw) to NHWC [M][HW][C]. */
int sst_linear_ksplit(int M, int N, int K);
int sst_linear_fwd(const float* x, const float* w, const float* bias, float* y, float* slab, int M, int N,
                   int K, void* stream);
int sst_linear_dgrad(const float* dy, const float* w, float* dx, int M, int N, int K, int nhwc_C,
                     int nhwc_HW, void* stream);
int sst_linear_wgrad(const float* dy, const float* x, float* dw, float* db, int M, int N, int K,
                     int accumulate, void* stream);
int sst_head_fwd(const float* h, const float* w, const float* b, float* y, int M, int N, int K, float slope,
                 void* stream);
int sst_head_bwd(const float* h, const float* w, const float* dy, float* dh, float* dw, float* db, int M,
                 int N, int K, float slope, int accumulate, void* stream);
/* scale / shift [B / grp_images][C] (passes batched as one tensor); grp_images = 0: one row */
int sst_flatten_act_grp(const float* y, const float* scale, const float* shift, float slope, int act,
                        float* flat, int B, int HW, int C, int grp_images, void* stream);

/* ---- optimizer: torch.optim.Adam(lr, betas, eps=1e-4) of train.py:62-75 / warmup.py:34-40 as ONE streaming pass over
 * flat parameter / gradient / moment buffers (n floats, n % 4 == 0).  steps: nsteps device floats, all incremented by
 * one (the per-parameter `step` tensors of torch's optimizer state); lr: device scalar (LR schedulers fill it). */
int sst_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, float* steps,
                  int nsteps, double beta1, double beta2, double eps, double weight_decay, void* stream);

/* sst_adam_flat plus, in the same pass, an exponential moving average of the parameters: with t = steps[0] after the tick,
 * d = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay and ema = (float)(d * ema + (1 - d) * p_new), evaluated
 * in double.  ema: n floats in p's layout.  p / m / v come out bit-identical to sst_adam_flat's. */
int sst_adam_flat_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* lr, float* steps,
                      int nsteps, double beta1, double beta2, double eps, double weight_decay, double ema_decay,
                      int ema_warmup, void* stream);

/* The average's update alone (no tick, no Adam) with t = steps[0] as it stands: for steps whose Adam update ran elsewhere. */
int sst_ema_flat(float* ema, const float* p, int64_t n, const float* steps, double ema_decay, int ema_warmup, void* stream);

/* ---- global gradient-norm clipping and the non-finite step guard on the same flat buffers.
 * sst_grad_sumsq: fp64 sum of squares of the PARAMETER elements of a flat gradient buffer g (n floats, 16-byte aligned).  The
 * pad words between parameter slots are never read: the kernel is driven by a job table of njobs (start, count) int64 pairs,
 * one workgroup per job, partials[j] = sum of g[start .. start + count)^2 with every value widened to double before it is
 * squared.  jobs is the table in device memory, jobs_host the same table in host memory; the host copy is checked (count > 0,
 * 0 <= start, start + count <= n) before anything is launched.  Fixed order, no atomics: bit-reproducible. */
int sst_grad_sumsq(const float* g, int64_t n, const int64_t* jobs, const int64_t* jobs_host, int njobs, double* partials,
                   void* stream);

/* sst_adam_flat (ema == NULL) or sst_adam_flat_ema with the clip rule, two launches.  The first sums partials[0 .. npartials)
 * (sst_grad_sumsq's output for g) in a fixed order and writes the record rec[6] (doubles): norm = sqrt(sum); coef =
 * (float)min(1, max_norm / (norm + 1e-6)) evaluated in double (max_norm == 0: no clipping, coef = 1; a NaN norm gives a NaN
 * coef, as torch.nn.utils.clip_grad_norm_ does); skipped_now = skip_nonfinite && the sum is not finite; and the cumulative
 * n_skipped, n_clipped, n_steps_seen (rec is zeroed once by the caller).  The step counters tick only when not skipping.  The
 * second is the update: on skip p / m / v / ema are not touched, otherwise each gradient element is g * coef (one fp32
 * multiply) and the rest is sst_adam_flat's arithmetic - with coef == 1 its bits. */
int sst_adam_flat_clip(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* lr, float* steps,
                       int nsteps, double beta1, double beta2, double eps, double weight_decay, double ema_decay,
                       int ema_warmup, const double* partials, int npartials, double max_norm, int skip_nonfinite,
                       double* rec, void* stream);

#ifdef __cplusplus
}
#endif
#endif
