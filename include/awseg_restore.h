/*
 * awseg_restore.h — input-restoration entry points of libawseg_hip.so.  An extension header: same conventions as
 * awseg.h (device pointers unless documented "host", stream-ordered, no allocation, no synchronisation, 0 / hipError_t / AWSEG_E*),
 * whose types and error codes it uses.  awseg_abi_version stays what awseg.h says; the bindings keep these symbols in a table of
 * their own (_native.EXTENSION_SIGNATURES).
 */
#ifndef AWSEG_RESTORE_H
#define AWSEG_RESTORE_H

#include "awseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 60 bits of sha256 of THIS file as it was when the library was built, as awseg_header_hash is of awseg.h: a binding that finds
 * another hash beside the library refuses to call the entry points below. */
uint64_t awseg_restore_header_hash(void);

/* ------------------------------------------------------------------------- *
 *  Dark-channel-prior dehazing (He, Sun, Tang 2009) of the frames the model sees, as a blind front-end of the evaluation
 *       replaces nothing: the reference has no restoration baseline
 * ------------------------------------------------------------------------- *
 * awseg_dehaze: image float32 [B, 3, H, W], the loader's normalised frames; mean, std: HOST float32[3] (they travel in the kernel
 * arguments).  radius r in [1, 15] (windows are (2r+1)^2, clipped to the frame: positions outside take part in no minimum and no
 * maximum), omega, t_min, airlight_min in (0, 1], refine 0 or 1.  Every step is one float32 operation with the parenthesisation
 * given (the library is built without FMA contraction, float32 and float64 division are correctly rounded), so numpy gives the
 * same bits.  Per frame b, pixel p, channel c:
 *     v_c  = fminf(fmaxf(image[b,c,p] * std[c] + mean[c], 0), 1)         (NaN -> 0; every input value that is not finite is counted)
 *   pass A   m = fminf(fminf(v_0, v_1), v_2);  dark = window minimum of m;  bin = (int)(dark * 255.0f), one uint8 per pixel in the
 *            workspace and one count in the frame's 256-bin histogram
 *   pass B   n_top = (H*W + 999) / 1000 (integers);  b* = the largest bin with sum_{k >= b*} hist[k] >= n_top;  over the pixels with
 *            bin >= b*:  S_c += (int64) rintf(v_c * 65536.0f),  N += 1;
 *            a_c = (float)((double) S_c / ((double) N * 65536.0));  A_c = fmaxf(a_c, airlight_min);  the frame's airlight "hit the
 *            floor" when a_c < airlight_min for some c
 *   pass C   n = fminf(fminf(v_0 / A_0, v_1 / A_1), v_2 / A_2);  e = window minimum of n;
 *            o = e (refine 0), or the window maximum of e (refine 1: the morphological opening of n);
 *            t = fmaxf(1.0f - omega * o, t_min);
 *            J_c = fminf(fmaxf((v_c - A_c) / t + A_c, 0), 1);   restored[b,c,p] = (J_c - mean[c]) / std[c]
 * restored float32 [B, 3, H, W] (must not overlap image: a block reads its neighbours' pixels); airlight float32 [B][3] = A.
 * stats int64 [n_slots][AWSEG_DEHAZE_ROW] (accumulated, never cleared), slot rule of every other counter: frame b into slot 0 and
 * into slot 1 + cond[b] when 0 <= cond[b] < n_slots - 1 (cond device int32[B] or NULL: slot 0 only).  Row:
 *     [0] frames   [1..3] sum of rintf(A_c * 65536.0f), c = 0, 1, 2   [4] pixels   [5] sum of rintf(t * 65536.0f)
 *     [6] input values that are not finite   [7] frames whose airlight hit the floor
 * Integer sums only: independent of the grid, additive over launches and ranks.  A term is at most 2^16 units, so a stats tensor
 * holds 2^46 pixels before a sum could wrap.
 * Three kernels: A and C are tile kernels, a block owns AWSEG_DEHAZE_TILE_H x AWSEG_DEHAZE_TILE_W pixels and stages them with a halo
 * of r (A; C with refine 0) or 2 r (C with refine 1) in LDS, separable window passes there; B walks the bin map.  16-byte loads and
 * stores when W % 4 == 0 and image and restored are 16-byte aligned (four bins then travel as one 32-bit word), scalar ones otherwise.
 * workspace: awseg_dehaze_workspace(batch, height, width) bytes
 *     = batch * (AWSEG_DEHAZE_FRAME_RECORD + height * width):
 * per frame a record of 256 uint32 histogram words and five int64 (S_0, S_1, S_2, N, non-finite values), then one uint8 bin per
 * pixel; 8-byte aligned (AWSEG_EALIGN otherwise).  The launcher clears the records on the stream.
 * AWSEG_EINVAL for a NULL pointer (cond excepted), channels != 3, a size < 1 (batch < 0), n_slots < 1, a parameter outside the
 * ranges above (NaN included), a std that is not finite and > 0 or a non-finite mean; AWSEG_ERANGE for batch > 65535 or
 * H * W >= 2^31; batch == 0 returns 0. */
#define AWSEG_DEHAZE_ROW           8
#define AWSEG_DEHAZE_TILE_H        32
#define AWSEG_DEHAZE_TILE_W        64
#define AWSEG_DEHAZE_MAX_RADIUS    15
#define AWSEG_DEHAZE_FRAME_RECORD  1064
int64_t awseg_dehaze_workspace(int64_t batch, int64_t height, int64_t width);
int awseg_dehaze(const float* image, int64_t batch, int channels, int64_t height, int64_t width,
                 const float* mean, const float* std, int radius, float omega, float t_min, float airlight_min, int refine,
                 const int32_t* cond, float* restored, float* airlight, int64_t* stats, int n_slots,
                 void* workspace, awseg_stream_t stream);

/* ------------------------------------------------------------------------- *
 *  The same front-end with the guided-filter refinement of the transmission (He, Sun, Tang, "Guided Image Filtering", 2010/2013):
 *  the patch transmission filtered with the frame's own luma as the guide
 *       replaces nothing: the reference has no restoration baseline
 * ------------------------------------------------------------------------- *
 * awseg_dehaze_guided: image, mean, std, radius, omega, t_min, airlight_min, cond, restored, airlight, stats, n_slots as for
 * awseg_dehaze (which this entry point leaves as it is); guided_radius R in [1, AWSEG_GUIDED_MAX_RADIUS], guided_eps eps in
 * [1e-4, 1].  v_c, pass A, pass B and A_c are those of awseg_dehaze.  Then, one float32 operation per step, parenthesised as written,
 * no contraction:
 *     n = fminf(fminf(v_0 / A_0, v_1 / A_1), v_2 / A_2);   e = (2r+1)^2 window minimum of n (pass C with refine 0)
 *     p = 1.0f - omega * e                                  (the raw patch transmission, before any clamp)
 *     g = (0.299f * v_0 + 0.587f * v_1) + 0.114f * v_2      (the guide)
 *   the box sum S(x) of a map x over (2R+1)^2 windows, positions outside the frame being +0.0f:
 *     h[y,x] = ((x[y,x-R] + x[y,x-R+1]) + ...) + x[y,x+R]   left to right, 2R additions
 *     S[y,x] = ((h[y-R,x] + h[y-R+1,x]) + ...) + h[y+R,x]   top to bottom, 2R additions (rows outside the frame are rows of +0.0f)
 *     N[y,x] = (rows of the window inside the frame) * (columns of the window inside the frame), as float32 (exact);  M(x) = S(x) / N
 *   The order of the additions is part of the contract: a sliding-window or a tree sum gives other bits.
 *     mg = M(g);  mp = M(p);  mgg = M(g * g);  mgp = M(g * p)          (the products are taken per position, before the sums)
 *     var = mgg - mg * mg;  cov = mgp - mg * mp;  a = cov / (var + eps);  b = mp - a * mg
 *     q = M(a) * g + M(b)
 *     t = fmaxf(fminf(q, 1.0f), t_min);   J_c and restored[b,c,p] from t as in pass C;   transmission[b,p] = t
 * The lower bound of eps keeps var + eps > 0 under float32 cancellation (on values in [0, 1] the rounding of a window sum is about
 * 65 * 2^-24).  transmission float32 [B, H, W] or NULL (then t is not stored).
 * stats: the row of awseg_dehaze with the refined t in [5].  guided_stats int64 [n_slots][AWSEG_GUIDED_ROW], the same slot rule,
 * accumulated and never cleared:
 *     [0] pixels with q > 1.0f   [1] pixels with q < t_min   [2] sum of rintf(fabsf(t - fmaxf(p, t_min)) * 65536.0f): how far the
 *     filter moved the patch transmission   [3] pixels
 * Integer sums only.
 * Five kernels on the stream: A and B of awseg_dehaze; a coarse pass (pass C's staging and window minimum) that stores p; a
 * coefficient kernel (a block owns AWSEG_DEHAZE_TILE_H x AWSEG_DEHAZE_TILE_W pixels, stages g and p with a halo of R, forms the four
 * box sums one after another through one row-sum buffer, stores a and b); a final kernel (stages a and b with a halo of R, forms
 * M(a), M(b), then t, J, the outputs and the counters).  16-byte loads and stores of the frames when W % 4 == 0 and image, restored
 * and transmission are 16-byte aligned, scalar ones otherwise.
 * workspace: awseg_dehaze_guided_workspace(batch, height, width) bytes
 *     = ceil8(batch * (AWSEG_DEHAZE_FRAME_RECORD + height * width)) + 3 * ceil8(4 * batch * height * width),   ceil8(x) = (x + 7) & ~7:
 * the records and the bin map of awseg_dehaze, then the float32 maps p, a, b, [B, H, W] each, every region beginning on an 8-byte
 * boundary; 8-byte aligned (AWSEG_EALIGN otherwise).
 * Refusals: those of awseg_dehaze with the same codes; also AWSEG_EINVAL for guided_radius outside [1, AWSEG_GUIDED_MAX_RADIUS],
 * guided_eps outside [1e-4, 1] (NaN included) and a NULL guided_stats.  batch == 0 returns 0 and launches nothing. */
#define AWSEG_GUIDED_ROW         4
#define AWSEG_GUIDED_MAX_RADIUS  32
int64_t awseg_dehaze_guided_workspace(int64_t batch, int64_t height, int64_t width);
int awseg_dehaze_guided(const float* image, int64_t batch, int channels, int64_t height, int64_t width,
                        const float* mean, const float* std, int radius, float omega, float t_min, float airlight_min,
                        int guided_radius, float guided_eps, const int32_t* cond,
                        float* restored, float* airlight, float* transmission /* [B,H,W] or NULL */,
                        int64_t* stats /* [n_slots][AWSEG_DEHAZE_ROW] */, int64_t* guided_stats /* [n_slots][AWSEG_GUIDED_ROW] */,
                        int n_slots, void* workspace, awseg_stream_t stream);

/* ------------------------------------------------------------------------- *
 *  Night relighting: contrast-limited adaptive histogram equalisation of the luma (CLAHE; Zuiderveld 1994, the algorithm of
 *  OpenCV's createCLAHE) with a grey-world white balance, the second blind front-end of the evaluation
 *       replaces nothing: the reference has no restoration baseline
 * ------------------------------------------------------------------------- *
 * awseg_relight: image, mean, std (HOST float32[3]), cond, restored, stats, n_slots, workspace, stream as for awseg_dehaze (which
 * this entry point leaves as it is).  tiles_y, tiles_x in [1, AWSEG_RELIGHT_MAX_TILES], tiles_y <= H, tiles_x <= W; clip_limit and
 * max_gain in [1, 64]; white_balance 0 or 1.  Every step is one float32 operation with the parenthesisation given (no contraction,
 * correctly rounded division) unless it is written in integers or in double, so numpy gives the same bits.  Frame b, pixel (y, x):
 *   input    v_c = fminf(fmaxf(image[b,c,y,x] * std[c] + mean[c], 0), 1)   (NaN -> 0; every input value that is not finite is counted:
 *            the v_c of awseg_dehaze);   l = (0.299f * v_0 + 0.587f * v_1) + 0.114f * v_2;   bin = min((int)(l * 255.0f), 255)
 *   tiles    tile row i covers the rows [floor(i H / tiles_y), floor((i + 1) H / tiles_y)), tile column j the columns
 *            [floor(j W / tiles_x), floor((j + 1) W / tiles_x)): tiles need not be equal and are never empty.  No padding and no
 *            reflection: OpenCV pads the frame to a multiple of the grid, this does not, so the tables differ from OpenCV's wherever
 *            the grid does not divide the frame.
 *   pass A   per (frame, tile) the 256-bin histogram hist of bin (uint32); per frame S_c = sum of (int64) rintf(v_c * 65536.0f)
 *            and the count of the input values that are not finite
 *   pass B   per tile of n pixels, in integers except where written:
 *              L = max(1, (int)((clip_limit * (float) n) / 256.0f));   E = sum_k max(hist[k] - L, 0)
 *              h[k] = min(hist[k], L) + E / 256;   r = E % 256;   step = max(256 / r, 1) (r > 0):  h[0], h[step], h[2 step], ...
 *              each get one more until r are given (ONE redistribution pass, OpenCV's)
 *              cdf[k] = sum_{m <= k} h[m]  (cdf[255] == n);   lut[k] = (uint16)((cdf[k] * 65535 + n / 2) / n)  in 64-bit arithmetic
 *            per frame:  m_c = (float)((double) S_c / ((double)(H * W) * 65536.0));   grey = ((m_0 + m_1) + m_2) / 3.0f;
 *              k_c = fminf(fmaxf(grey / fmaxf(m_c, 1.0f / 256.0f), 0.25f), 4.0f), or 1.0f when white_balance == 0;  gains[b][c] = k_c
 *   pass C   cy_i = (float)(y0_i + y1_i - 1) * 0.5f, the centre of tile row i = rows [y0_i, y1_i).  i0 = the largest i with
 *            cy_i <= y (compared exactly, as integers: y0_i + y1_i - 1 <= 2 y).  None: i0 = i1 = 0, wy = 0.  i0 = tiles_y - 1: i1 = i0, wy = 0.  Otherwise i1 = i0 + 1 and
 *            wy = ((float) y - cy_i0) / (cy_i1 - cy_i0).  Columns likewise: j0, j1, wx.
 *            a, b, c, d = (float) lut[i0][j0][bin], lut[i0][j1][bin], lut[i1][j0][bin], lut[i1][j1][bin]
 *              top = a + wx * (b - a);   bot = c + wx * (d - c);   l' = (top + wy * (bot - top)) / 65535.0f
 *              raw = l' / fmaxf(l, 1.0f / 256.0f);   g = fminf(raw, max_gain)
 *              u_c = (v_c * k_c) * g;   J_c = fminf(fmaxf(u_c, 0), 1);   restored[b,c,y,x] = (J_c - mean[c]) / std[c]
 *            The table is indexed by the 8-bit bin, not interpolated within it: all pixels of one bin and one position weight get
 *            one output luma.  The frames come from 8-bit renderings, so nothing is lost there.
 * restored float32 [B, 3, H, W] (must not overlap image); gains float32 [B][3] = k.
 * stats int64 [n_slots][AWSEG_RELIGHT_ROW] (accumulated, never cleared), the slot rule of awseg_dehaze (slot 0, and slot
 * 1 + cond[b] when 0 <= cond[b] < n_slots - 1; cond device int32[B] or NULL).  Row:
 *     [0] frames   [1..3] sum of rintf(k_c * 65536.0f), c = 0, 1, 2   [4] pixels   [5] sum of rintf(l * 65536.0f)
 *     [6] sum of rintf(fminf(l_out, 1.0f) * 65536.0f), l_out = (0.299f * J_0 + 0.587f * J_1) + 0.114f * J_2
 *     [7] input values that are not finite   [8] pixels with raw > max_gain   [9] channel values with u_c > 1.0f
 * Integer sums only: independent of the grid, additive over launches and ranks.  A term is at most 2^18 units (a gain of 4), the
 * per-pixel terms at most 2^16, so a stats tensor holds 2^46 pixels (and 2^44 frames) before a sum could wrap.
 * On the stream: one clear of the records and histograms, then three kernels.  A and C are streaming passes over strips of rows
 * (16-byte loads and stores when W % 4 == 0 and image and restored are 16-byte aligned, scalar ones otherwise; the same bits either
 * way; a group of four pixels may straddle two tiles); A counts into LDS histograms and adds them to the tiles' words with integer
 * atomics; B is one 256-thread block per tile and one more per frame for the gains and the frame's counters; C stages the tables
 * of its two tile rows in LDS.
 * workspace: awseg_relight_workspace(batch, tiles_y, tiles_x) bytes
 *     = batch * (AWSEG_RELIGHT_FRAME_RECORD + tiles_y * tiles_x * AWSEG_RELIGHT_TILE_BYTES):
 * the frames' records (int64 S_0, S_1, S_2, non-finite values; float32 k_0, k_1, k_2 and a pad), then every tile's 256 uint32
 * histogram words, then every tile's 256 uint16 table entries; every region begins on an 8-byte boundary; 8-byte aligned
 * (AWSEG_EALIGN otherwise).  The launcher clears the records and the histograms on the stream.
 * AWSEG_EINVAL for a NULL pointer (cond excepted), channels != 3, a size < 1 (batch < 0), n_slots < 1, a grid outside
 * [1, AWSEG_RELIGHT_MAX_TILES] or larger than the frame, clip_limit or max_gain outside [1, 64] (NaN included), white_balance other
 * than 0 or 1, a std that is not finite and > 0 or a non-finite mean; AWSEG_ERANGE for batch > 65535 or H * W >= 2^31;
 * batch == 0 returns 0 and launches nothing. */
#define AWSEG_RELIGHT_ROW           10
#define AWSEG_RELIGHT_MAX_TILES     16
#define AWSEG_RELIGHT_FRAME_RECORD  48
#define AWSEG_RELIGHT_TILE_BYTES    1536
int64_t awseg_relight_workspace(int64_t batch, int tiles_y, int tiles_x);
int awseg_relight(const float* image, int64_t batch, int channels, int64_t height, int64_t width,
                  const float* mean, const float* std, int tiles_y, int tiles_x, float clip_limit, float max_gain,
                  int white_balance, const int32_t* cond, float* restored, float* gains /* [B][3] */,
                  int64_t* stats /* [n_slots][AWSEG_RELIGHT_ROW] */, int n_slots, void* workspace, awseg_stream_t stream);

/* ------------------------------------------------------------------------- *
 *  Rain and snow removal: bright occluders narrower than a window found by the morphological white top-hat of every channel and
 *  filled from their unmasked neighbours, the third blind front-end of the evaluation
 *       replaces nothing: the reference has no restoration baseline
 * ------------------------------------------------------------------------- *
 * awseg_deocclude: image, mean, std (HOST float32[3]), cond, restored, stats, n_slots, workspace, stream as for awseg_dehaze (which
 * this entry point leaves as it is).  radius r in [1, AWSEG_DEHAZE_MAX_RADIUS], threshold in (0, 1], bright_min in [0, 1], dilate d
 * in [0, AWSEG_DEOCCLUDE_MAX_DILATE].  Every float step is one float32 operation with the parenthesisation given (no contraction);
 * everything else is written in integers or in double, so numpy gives the same bits.  All windows are clipped to the frame:
 * positions outside take part in no minimum, no maximum and no sum.  Frame b, pixel p, channel c:
 *   input    v_c = fminf(fmaxf(image[b,c,p] * std[c] + mean[c], 0), 1)     (NaN -> 0; every input value that is not finite is counted:
 *            the v_c of awseg_dehaze)
 *   pass A   e_c = (2r+1)^2 window minimum of v_c;   o_c = (2r+1)^2 window maximum of e_c   (the opening of v_c: o_c <= v_c)
 *            h = fminf(fminf(v_0 - o_0, v_1 - o_1), v_2 - o_2)             (the smallest of the three white top-hats)
 *            b = fminf(fminf(v_0, v_1), v_2)
 *            seed = (h > threshold) && (b >= bright_min)      a near-white occluder lifts all three channels over their opened
 *                                                             background, a thin coloured object does not
 *            mask = (2d+1)^2 window maximum of seed           (covers the blurred rim);   mask[b,p] = 0 or 1, one uint8
 *   pass B   q_c = (int32) rintf(v_c * 65536.0f)
 *            over the (2r+1)^2 window: N = the count of the positions with mask == 0, S_c = the integer sum of q_c over them
 *            (S_c <= 961 * 2^16 < 2^26; integers, so the order is free)
 *            mask == 1 and N > 0:   J_c = (float)((double) S_c / ((double) N * 65536.0))
 *            mask == 1 and N == 0:  J_c = v_c   (the pixel is "left unfilled")
 *            mask == 0:             J_c = v_c
 *            restored[b,c,p] = (J_c - mean[c]) / std[c]
 * restored float32 [B, 3, H, W] (must not overlap image: a block reads its neighbours' pixels); mask uint8 [B, H, W].
 * stats int64 [n_slots][AWSEG_DEOCCLUDE_ROW] (accumulated, never cleared), the slot rule of awseg_dehaze (slot 0, and slot
 * 1 + cond[b] when 0 <= cond[b] < n_slots - 1; cond device int32[B] or NULL).  Row:
 *     [0] frames   [1] pixels   [2] seed pixels   [3] masked pixels   [4] masked pixels left unfilled
 *     [5] sum over the masked pixels and the channels of |(int64) rintf(J_c * 65536.0f) - q_c|   [6] input values that are not finite
 * Integer sums only: independent of the grid, additive over launches and ranks.  A term is at most 3 * 2^16 units, so a stats
 * tensor holds 2^44 pixels before a sum could wrap.
 * Two kernels on the stream, both on the AWSEG_DEHAZE_TILE_H x AWSEG_DEHAZE_TILE_W tiles of awseg_dehaze.  The detection kernel
 * walks the three channels one after another through one staged plane with a halo of 2 r + d (at most 32) and one scratch plane,
 * separable row and column passes in LDS, keeping the running minimum of the top-hats in registers; then it dilates the seeds and
 * writes the mask.  The fill kernel walks the channels again with a halo of r: it stages q_c of the unmasked positions with their
 * count in the upper bits of the same word, and forms separable integer window sums.  16-byte loads and stores of the frames and
 * 32-bit ones of the mask when W % 4 == 0, image and restored are 16-byte aligned and mask is 4-byte aligned, scalar ones
 * otherwise; the same bits either way.
 * workspace: awseg_deocclude_workspace(batch, height, width) bytes = 0: the only thing one kernel leaves for the other is the mask,
 * which is an output.  So the pointer may be NULL, as a buffer of no bytes is; one that is given is 8-byte aligned as elsewhere
 * (AWSEG_EALIGN otherwise) and never dereferenced.
 * AWSEG_EINVAL for a NULL pointer (cond and workspace excepted), channels != 3, a size < 1 (batch < 0), n_slots < 1, a parameter outside the
 * ranges above (NaN included), a std that is not finite and > 0 or a non-finite mean; AWSEG_ERANGE for batch > 65535 or
 * H * W >= 2^31; batch == 0 returns 0 and launches nothing. */
#define AWSEG_DEOCCLUDE_ROW         7
#define AWSEG_DEOCCLUDE_MAX_DILATE  2
int64_t awseg_deocclude_workspace(int64_t batch, int64_t height, int64_t width);
int awseg_deocclude(const float* image, int64_t batch, int channels, int64_t height, int64_t width,
                    const float* mean, const float* std, int radius, float threshold, float bright_min, int dilate,
                    const int32_t* cond, float* restored, uint8_t* mask /* [B,H,W] */,
                    int64_t* stats /* [n_slots][AWSEG_DEOCCLUDE_ROW] */, int n_slots, void* workspace, awseg_stream_t stream);

/* ------------------------------------------------------------------------- *
 *  Weather estimate: which of the three front-ends above a frame needs, decided per frame from its pixels alone, for the blind
 *  routing of the evaluation
 *       replaces nothing: the reference has no restoration baseline
 * ------------------------------------------------------------------------- *
 * awseg_weather_estimate: image, mean, std (HOST float32[3]), cond, stats, n_slots, workspace, stream as for awseg_dehaze (which
 * this entry point leaves as it is, as it leaves awseg_relight and awseg_deocclude).  radius r in [1, AWSEG_DEHAZE_MAX_RADIUS],
 * threshold in (0, 1], bright_min in [0, 1] (those of awseg_deocclude); cast_max in (0, 4], luma_max in (0, 1], dark_min in [0, 1),
 * seed_min in [0, 1).  Every float step is one float32 operation with the parenthesisation given (no contraction); everything else
 * is written in integers or in double, so numpy gives the same bits.  All windows are clipped to the frame.  Frame b, pixel p:
 *   input    v_c = fminf(fmaxf(image[b,c,p] * std[c] + mean[c], 0), 1)     (NaN -> 0; every input value that is not finite is counted:
 *            the v_c of awseg_dehaze)
 *   pixel    e_c = (2r+1)^2 window minimum of v_c;   o_c = (2r+1)^2 window maximum of e_c
 *            m = fminf(fminf(v_0, v_1), v_2);   h = fminf(fminf(v_0 - o_0, v_1 - o_1), v_2 - o_2)
 *            seed = (h > threshold) && (m >= bright_min)                   (pass A of awseg_deocclude before the dilation)
 *            dark = (2r+1)^2 window minimum of m                           (pass A of awseg_dehaze before the binning; the kernel forms
 *                                                                          it as fminf(fminf(e_0, e_1), e_2): minima commute)
 *            l = (0.299f * v_0 + 0.587f * v_1) + 0.114f * v_2
 *   frame    Q_dark = sum of (int64) rintf(dark * 65536.0f);  Q_l from l and Q_c from v_c (c = 0, 1, 2) likewise;  N_seed = the
 *            count of seeds;  the count of the input values that are not finite
 *            P = (double)(H * W) * 65536.0;   D = (float)((double) Q_dark / P);   L = (float)((double) Q_l / P);
 *            M_c = (float)((double) Q_c / P);   O = (float)((double) N_seed / (double)(H * W))
 *   route    the first rule that matches, float32 compares (cast_max * M_2 is one float32 product):
 *              1. (M_0 < cast_max * M_2) && (L < luma_max)  ->  2   a dark frame with a blue cast: awseg_relight
 *              2. D > dark_min                              ->  1   a veil: awseg_dehaze
 *              3. O > seed_min                              ->  3   bright occluders: awseg_deocclude
 *              4. otherwise                                 ->  0   nothing
 *            The veil comes before the occluders: a fog frame carries top-hat seeds of its own.
 * route int32 [B]; descriptors float32 [B][AWSEG_ESTIMATE_DESCRIPTORS] = D, L, M_0, M_1, M_2, O.
 * stats int64 [n_slots][AWSEG_ESTIMATE_ROW] (accumulated, never cleared), the slot rule of awseg_dehaze (slot 0, and slot
 * 1 + cond[b] when 0 <= cond[b] < n_slots - 1; cond device int32[B] or NULL).  Row:
 *     [0] frames   [1] pixels   [2] sum of Q_dark   [3] sum of Q_l   [4..6] sum of Q_c, c = 0, 1, 2   [7] seed pixels
 *     [8] input values that are not finite   [9..12] frames routed to 0, 1, 2, 3
 * Integer sums only: independent of the grid, additive over launches and ranks.  A term is at most 2^16 units, so a stats tensor
 * holds 2^46 pixels before a sum could wrap.  With cond the true condition, [9..12] of the slots are the confusion table of the
 * estimate.
 * On the stream: one clear of the records, then two kernels.  The first runs on the AWSEG_DEHAZE_TILE_H x AWSEG_DEHAZE_TILE_W tiles
 * of awseg_dehaze and is the detection kernel of awseg_deocclude at d = 0 without the dilation and the mask: the three channels one
 * after another through one staged plane with a halo of 2 r and one scratch plane, separable passes in LDS, the running minima in
 * registers, one block-level reduction and one 64-bit atomic per quantity and block into the frame's record.  The second, one
 * thread per frame, forms the descriptors and the route and adds the frame's row to its slots.  16-byte loads when W % 4 == 0 and
 * image is 16-byte aligned, scalar ones otherwise; the same bits either way.
 * workspace: awseg_weather_estimate_workspace(batch) bytes = batch * AWSEG_ESTIMATE_FRAME_RECORD: per frame seven int64 (Q_dark,
 * Q_l, Q_0, Q_1, Q_2, N_seed, non-finite values) and a pad; 8-byte aligned (AWSEG_EALIGN otherwise).  The launcher clears it on the
 * stream.
 * AWSEG_EINVAL for a NULL pointer (cond excepted), channels != 3, a size < 1 (batch < 0), n_slots < 1, a parameter outside the
 * ranges above (NaN included), a std that is not finite and > 0 or a non-finite mean; AWSEG_ERANGE for batch > 65535 or
 * H * W >= 2^31; batch == 0 returns 0 and launches nothing. */
#define AWSEG_ESTIMATE_ROW           13
#define AWSEG_ESTIMATE_DESCRIPTORS   6
#define AWSEG_ESTIMATE_FRAME_RECORD  64
int64_t awseg_weather_estimate_workspace(int64_t batch);
int awseg_weather_estimate(const float* image, int64_t batch, int channels, int64_t height, int64_t width,
                           const float* mean, const float* std, int radius, float threshold, float bright_min,
                           float cast_max, float luma_max, float dark_min, float seed_min, const int32_t* cond,
                           int32_t* route /* [B] */, float* descriptors /* [B][AWSEG_ESTIMATE_DESCRIPTORS] */,
                           int64_t* stats /* [n_slots][AWSEG_ESTIMATE_ROW] */, int n_slots, void* workspace, awseg_stream_t stream);

/* ------------------------------------------------------------------------- *
 *  Test-time augmentation: the two steps between the forwards of a prediction averaged over mirrored and rescaled views of the
 *  same frames ("ms+flip")
 *       replaces nothing: the reference evaluates one view
 * ------------------------------------------------------------------------- *
 * Both work on planar float32 maps, source [B, C, h, w] and destination [B, C, H, W], and sample bilinearly with
 * align_corners = False.  Every step is one float32 operation in the order written, no contraction, so numpy float32 gives the same
 * bits (this is NOT the fmaf form of awseg_upsample_bilinear, which is pinned to torch's build):
 *     sy = (float) h / (float) H,  sx = (float) w / (float) W                 (on the host)
 *     f   = fmaxf(sy * ((float) y + 0.5f) - 0.5f, 0)                          (add, multiply, subtract, max)
 *     y0  = min((int) f, h - 1);   y1 = y0 + (y0 < h - 1);   ly1 = f - (float) y0;   ly0 = 1.0f - ly1          (columns likewise)
 *     top = lx0 * v00 + lx1 * v01;   bot = lx0 * v10 + lx1 * v11;   U = ly0 * top + ly1 * bot      (products, then the sum)
 * with v_ij the source value at (y_i, x_j).  A product whose weight is exactly 0 is replaced by +0.0f: a neighbour that is not
 * finite and takes no part (the second tap where f is whole, as at the first row and column) does not turn the pixel into NaN.  When
 * h == H and w == W, U is the source value itself, bit for bit, with no blend at all (so one inf in gives one inf out, and -0 stays).
 *
 * awseg_tta_view: dst[b,c,y,x] = U(y, flip ? W - 1 - x : x) of src: the frames resampled to (H, W), then mirrored.  channels in
 * [1, AWSEG_TTA_VIEW_MAX_CHANNELS].
 * awseg_tta_accumulate: U(y, x) is the sample at the frame pixel (y, x) of the map L'[r, c] = src[b, ch, r, flip ? w - 1 - c : c]:
 * the view's logits are mirrored back FIRST and resampled then, interpolate(flip(L)) and not flip(interpolate(L)), which differ in
 * bits.  Then, each product and each sum rounded on its own:
 *     AWSEG_TTA_SET        acc = weight * U
 *     AWSEG_TTA_ADD        acc = acc + weight * U
 *     AWSEG_TTA_SCALE_ADD  acc = weight * acc + weight * U      (the first extra view folded into the plain logits in place)
 * One streaming kernel: a lane owns four consecutive destination pixels of a row; 16-byte loads and stores of the destination when
 * W % 4 == 0 and it is 16-byte aligned, and at equal size of the source too when that is aligned (a mirrored group is one 16-byte
 * load with its components reversed); scalar accesses otherwise, the same bits either way.  The grid is capped and strided.  No
 * workspace, no LDS.
 * AWSEG_EINVAL for a NULL pointer, a size below 1 (batch and channels included), more view channels than
 * AWSEG_TTA_VIEW_MAX_CHANNELS, flip other than 0 or 1, an unknown mode, a weight that is not finite, or src == dst / src == acc;
 * AWSEG_EALIGN for a pointer that is not 4-byte aligned (16-byte accesses are used only where the pointers allow them);
 * AWSEG_ERANGE for a plane of 2^31 pixels or more, or B * C * H * ceil(W / 4) >= 2^31.  Refusals come before any launch. */
#define AWSEG_TTA_SET                0
#define AWSEG_TTA_ADD                1
#define AWSEG_TTA_SCALE_ADD          2
#define AWSEG_TTA_VIEW_MAX_CHANNELS  4
int awseg_tta_view(const float* src, int64_t batch, int channels, int64_t src_height, int64_t src_width,
                   float* dst /* [B,C,height,width] */, int64_t height, int64_t width, int flip, awseg_stream_t stream);
int awseg_tta_accumulate(const float* src, int64_t batch, int channels, int64_t src_height, int64_t src_width,
                         float* acc /* [B,C,height,width] */, int64_t height, int64_t width, int flip, float weight, int mode,
                         awseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AWSEG_RESTORE_H */
