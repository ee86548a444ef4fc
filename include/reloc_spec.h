/* reloc_spec.h -- numeric constants of the relocalization hot path.
 *
 * Constants only (no arithmetic): the CPU oracle (oracle/) and the HIP product library
 * (nclt-slam-project_amd/csrc/) each implement the stages independently and are held
 * bit-exact to each other by tests/.  Every constant cites the reference call site that
 * fixes it (paths relative to the reference repository root) or, where the arithmetic
 * lives inside OpenCV (absent from the reference tree and from this container), the
 * SURVEY.md Appendix A paragraph that restates OpenCV's published algorithm.
 */
#ifndef RELOC_SPEC_H
#define RELOC_SPEC_H

/* ORB_create(nfeatures=500): every other parameter left at OpenCV's default
 * (simulation/isaac/scripts/common/visual_landmark_matcher.py:207,
 *  simulation/isaac/scripts/common/visual_landmark_recorder.py:159). */
#define RELOC_ORB_NLEVELS        8
#define RELOC_ORB_SCALE_FACTOR   1.2          /* level scale = (float)pow(1.2, level)          */
#define RELOC_ORB_EDGE           31           /* edgeThreshold: keep 31 <= x < w-31             */
#define RELOC_ORB_PATCH          31           /* KeyPoint.size = 31 * scale                     */
#define RELOC_ORB_HALF_PATCH     15           /* intensity-centroid disc radius                 */
#define RELOC_FAST_THRESHOLD     20           /* fastThreshold                                  */
#define RELOC_FAST_ARC           9            /* FAST-9/16                                      */
#define RELOC_HARRIS_BLOCK       7            /* HARRIS_BLOCK_SIZE                              */
#define RELOC_HARRIS_K           0.04f
/* Capacity of the per-level "best 2*quota by FAST score, ties kept" set.  If more pixels
 * than this reach the cut score the cut is raised one score at a time until the set fits
 * (decided from the score histogram alone, so the rule is order-independent). */
#define RELOC_ORB_STAGE1_CAP     4096

/* BGR->gray 8-bit fixed point.  Two published OpenCV conventions, chosen by reloc_params.gray_coeff_bits:
 *   15 (DEFAULT since round 4; OpenCV 4.x 8-bit path, `gray_shift`): Y = (B*3735 + G*19235 + R*9798 + 16384) >> 15
 *   14 (OpenCV <= 3.x, `yuv_shift`):                  Y = (B*1868 + G*9617 + R*4899 + 8192)  >> 14
 * The reference can only run on OpenCV >= 4.8 (datasets/nclt/requirements.txt:3; ROS 2 Jazzy / NumPy-2-era wheel: >= 4.10), so the
 * call it makes at M:305 / R:240 computes the 15-bit form.  The two differ by +-1 on some pixels.  Neither can be checked against
 * OpenCV offline (parity unpinned). */
#define RELOC_GRAY_CB            1868
#define RELOC_GRAY_CG            9617
#define RELOC_GRAY_CR            4899
#define RELOC_GRAY_SHIFT         14
#define RELOC_GRAY15_CB          3735
#define RELOC_GRAY15_CG          19235
#define RELOC_GRAY15_CR          9798
#define RELOC_GRAY15_SHIFT       15
#define RELOC_GRAY_DEFAULT_BITS  RELOC_GRAY15_SHIFT
/* order argument of the gray stage: bit 0 = channel order (RELOC_ORDER_RGB), bit 1 = the 15-bit coefficient set */
#define RELOC_GRAY_FLAG_15BIT    2

/* 7x7 sigma=2 Gaussian in 8 fractional bits, sum == 256.  Horizontal pass in
 * 8.8 fixed point, vertical pass in 16.16, result = (v + 32768) >> 16, BORDER_REFLECT_101. */
#define RELOC_BLUR_K0            18
#define RELOC_BLUR_K1            33
#define RELOC_BLUR_K2            49
#define RELOC_BLUR_K3            56

/* INTER_LINEAR_EXACT restatement: 8 fractional bits per axis coefficient. */
#define RELOC_RESIZE_COEF_BITS   8

/* fastAtan2 polynomial, degrees; evaluated in float without fused multiply-add. */
#define RELOC_ATAN2_P1           57.283627f   /*  0.9997878412794807 * 180/pi */
#define RELOC_ATAN2_P3          (-18.667446f) /* -0.3258083974640975 * 180/pi */
#define RELOC_ATAN2_P5           8.9140005f   /*  0.1555786518463281 * 180/pi */
#define RELOC_ATAN2_P7          (-2.5397246f) /* -0.04432655554792128 * 180/pi */
#define RELOC_ATAN2_EPS          2.220446049250313e-16f  /* (float)DBL_EPSILON */
#define RELOC_DEG2RAD_F          0.017453292519943295f   /* (float)(pi/180)     */

/* Matcher gates (visual_landmark_matcher.py:56-76). */
#define RELOC_CANDIDATE_RADIUS_M 8.0
#define RELOC_MAX_CANDIDATES     5
#define RELOC_HEADING_TOL_DEG    90.0
#define RELOC_MIN_MATCHES        10
#define RELOC_MIN_INLIERS        10
#define RELOC_REPROJ_MAX_PX      2.0
#define RELOC_RANSAC_REPROJ_PX   3.0
#define RELOC_RANSAC_ITERATIONS  200
#define RELOC_RANSAC_CONFIDENCE  0.99         /* cv2.solvePnPRansac default */
#define RELOC_CONSISTENCY_M      5.0
/* Global-relocalisation variant (experiments/63_global_reloc/scripts/visual_landmark_matcher.py) */
#define RELOC_GLOBAL_MAX_CANDIDATES 25
#define RELOC_GLOBAL_MIN_INLIERS    18        /* :85 */
#define RELOC_GLOBAL_REPROJ_MAX_PX  1.5       /* :86 */
/* Accumulation (visual_landmark_matcher.py:85-89, :461). */
#define RELOC_ACCUM_MIN_DIST_M   5.0
#define RELOC_ACCUM_MIN_KPTS     30
#define RELOC_ACCUM_DEPTH_MIN_M  0.5
#define RELOC_ACCUM_DEPTH_MAX_M  15.0

/* Pinhole intrinsics (visual_landmark_matcher.py:49-52, visual_landmark_recorder.py:55-57). */
#define RELOC_FX 320.0
#define RELOC_FY 320.0
#define RELOC_CX 320.0
#define RELOC_CY 240.0

/* Recorder gates (visual_landmark_recorder.py:59-71, :270). */
#define RELOC_DEPTH_MIN_M        0.5f
#define RELOC_DEPTH_MAX_M        15.0f
#define RELOC_DEPTH_VAR_MAX_M    0.30f
#define RELOC_GROUND_Y_THRESHOLD 180
#define RELOC_MIN_RECORD_KPTS    30

/* Hypothesis sampler shared by oracle and product so both score the same hypothesis list
 * (SURVEY.md A.8 hazard 5): splitmix64 counter stream, four distinct indices per hypothesis. */
#define RELOC_RNG_GOLDEN         0x9E3779B97F4A7C15ull
#define RELOC_RNG_MUL1           0xBF58476D1CE4E5B9ull
#define RELOC_RNG_MUL2           0x94D049BB133111EBull
#define RELOC_PNP_SAMPLE         4            /* 3 for P3P + 1 to pick among its <=4 roots */
#define RELOC_LM_MAX_TRIALS      30
#define RELOC_LM_LAMBDA0         1e-3
/* Levenberg-Marquardt stops after the step that is smaller than STEP_EPS (rad / m) or changes the cost by less than
 * COST_EPS * cost.  The iteration converges quadratically from a RANSAC pose (steps 1e-2, 5e-5, 5e-8, 3e-11 on typical
 * problems), so a step below 1e-4 leaves an error of ~1e-8 -- four orders below the 1e-4 m / 1e-4 rad tolerance of the
 * north star; rounds 1-2 iterated to 1e-10 / 1e-13, two more trials (~7 us of a single-wave kernel) for digits nobody reads. */
#define RELOC_LM_STEP_EPS        1e-4
#define RELOC_LM_COST_EPS        1e-8         /* stop when |cost change| <= this * cost */
/* Resolvent cubic of the P3P quartic: Halley iteration from a Fujiwara-type upper bound, inside the bracket [0, hi] with a
 * bisection fallback, at most this many steps (rounds 1-2: Newton from the coefficient bound until x stopped moving, up to
 * 80 steps -- mean 32, 95th percentile 68, and a wave waits for its slowest lane).  The quartic's roots are polished on the
 * quartic itself afterwards, so the resolvent root needs no more. */
#define RELOC_P3P_CUBIC_ITERS    16

/* Lens distortion: OpenCV's default ("plumb_bob", Brown-Conrady) model with (k1, k2, p1, p2, k3), restated from OpenCV 4.x
 * (cv::projectPoints, cv::undistortPoints; not pinned against a cv2 build).  All in double.
 *   forward   x = X/Z, y = Y/Z, r2 = x^2 + y^2, rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3
 *             xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),  yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y,  u = fx xd + cx, v = fy yd + cy
 *   inverse   x0 = (u - cx) * (1/fx), y0 = (v - cy) * (1/fy) (OpenCV multiplies by the reciprocal); x = x0, y = y0; then
 *             UNDISTORT_ITERS times (cv::undistortPoints' default criteria, no epsilon test):
 *               r2 = x^2 + y^2, icdist = 1 / (1 + ((k3 r2 + k2) r2 + k1) r2); icdist < 0: (x, y) = (x0, y0), stop
 *               x = (x0 - (2 p1 x y + p2 (r2 + 2 x^2))) icdist,  y = (y0 - (p1 (r2 + 2 y^2) + 2 p2 x y)) icdist
 * PnP-RANSAC: P3P on undistorted normalized points, the fourth point picks the root by the ideal pixel K undistort(img);
 * scoring, inlier list, Levenberg-Marquardt and the mean error measure in distorted pixels through the forward model.
 * Recording / accumulation: X = x_u z, Y = y_u z with (x_u, y_u) = undistort(rounded pixel).  All-zero coefficients select
 * the pinhole kernels. */
#define RELOC_UNDISTORT_ITERS    5

/* CLAHE: cv2.createCLAHE(clipLimit, tileGridSize=(tx, ty)).apply(gray) on 8-bit single-channel input, restated from OpenCV 4.x
 * modules/imgproc/src/clahe.cpp (the reference: experiments/35_road_obstacle_avoidance/scripts/robust_anchor_localizer.py:50,103
 * and the teach / repeat phases of run_husky_teach_then_repeat.py, clipLimit=2.0, tileGridSize=(8, 8); not pinned against a
 * cv2 build).  w x h image, tx x ty tiles:
 *   tiles      w % tx == 0 && h % ty == 0: tile = (w / tx) x (h / ty) of the source.  Otherwise BOTH axes are padded at the
 *              right / bottom by tx - w % tx columns and ty - h % ty rows (a full extra tile on an axis that divides) with
 *              BORDER_REFLECT_101 (repeated for pads larger than the image, a 1-pixel axis maps to 0) and tile = padded / grid.
 *              Histograms read the padded image; the interpolation runs over the original w x h.
 *   clip       area = tile_w * tile_h; clipLimit > 0: clip = max((int)(clipLimit * area / 256), 1) in double; else no clip.
 *   redistribute  clipped = sum max(hist[i] - clip, 0), bins capped at clip; every bin += clipped / 256; then bins 0, step,
 *              2 step, ... get +1 while residual = clipped % 256 lasts, step = max(256 / residual, 1).
 *   LUT        lutScale = 255.0f / area (float division); lut[i] = saturate_cast<uchar>((float)sum_{j<=i} hist[j] * lutScale)
 *              (cvRound: half to even).
 *   interpolate   f32, no FMA: txf = x * (1.0f / tile_w) - 0.5f, tx1 = floor(txf), xa = txf - tx1, xa1 = 1.0f - xa,
 *              tx2 = min(tx1 + 1, tx - 1), tx1 = max(tx1, 0); the same in y; out = saturate_cast<uchar>((L11[v] xa1 + L12[v] xa)
 *              ya1 + (L21[v] xa1 + L22[v] xa) ya) with L<row><col> the LUTs of tiles (ty1|ty2, tx1|tx2), in this order. */
#define RELOC_CLAHE_BINS         256
#define RELOC_CLAHE_MAX_TILES    64   /* per grid dimension (reloc_set_clahe, reloc_clahe_u8) */

/* REMAP: cv2.remap(src, map1, map2, INTER_LINEAR | INTER_NEAREST, BORDER_CONSTANT, borderValue) on 8-bit images (nearest also
 * 16-bit), cv2.convertMaps and the map builders, restated from OpenCV 4.x modules/imgproc/src/imgwarp.cpp and
 * modules/calib3d/src/undistort.dispatch.cpp / fisheye.cpp (the reference: datasets/nclt/scripts/run_all_visual_slam.py:182,217,
 * datasets/rover/scripts/rectify_t265_stereo.py:113-156; not pinned against a cv2 build):
 *   fixed-point map   sx = cvRound(mapx * 32), sy = cvRound(mapy * 32): f32 product (exact), half to even, saturating to int32,
 *              NaN -> INT32_MIN (so NaN, +-inf and out-of-range values land outside every image);
 *              xy = (saturate_cast<short>(sx >> 5), saturate_cast<short>(sy >> 5)), arithmetic shifts;
 *              alpha = (sy & 31) * 32 + (sx & 31).  This is convertMaps(mapx, mapy, CV_16SC2) and what remap does with float
 *              maps.  The library stores and takes only this form.
 *   bilinear   taps p00 = src(y, x), p01 = src(y, x + 1), p10 = src(y + 1, x), p11 = src(y + 1, x + 1), (x, y) = xy,
 *              fx = alpha & 31, fy = alpha >> 5, weights 32 * {(32 - fx)(32 - fy), fx (32 - fy), (32 - fx) fy, fx fy} (sum 32768),
 *              dst = (p00 w0 + p01 w1 + p10 w2 + p11 w3 + (1 << 14)) >> 15, per channel.  OpenCV's weight table differs from the
 *              closed form in one entry (alpha 0: {32767, 0, 0, 1} after its saturate-and-fix-up step); the byte is the same
 *              for every alpha and every tap combination (|p11 - p00| < 2^14), tests/test_remap_host.py repeats the check.
 *   border     BORDER_CONSTANT only: each tap outside the source is replaced by the border value on its own.
 *   nearest    fixed-point map: the pixel at xy, the fraction ignored; float maps: (cvRound(mapx), cvRound(mapy)) saturated to
 *              short (convertMaps with nninterpolation); outside: the border value.
 *   builders   host, float64 (once per camera): initUndistortRectifyMap: (x, y, w) = (newK R)^-1 (u, v, 1), x' = x / w,
 *              y' = y / w, r2 = x'^2 + y'^2, kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2),
 *              xd = x' kr + 2 p1 x' y' + p2 (r2 + 2 x'^2) + s1 r2 + s2 r2^2, yd = y' kr + p1 (r2 + 2 y'^2) + 2 p2 x' y' + s3 r2 +
 *              s4 r2^2, tilt(tauX, tauY) applied to (xd, yd, 1), map = (fx xd + cx, fy yd + cy); CV_32FC1: cast to f32;
 *              CV_16SC2: iu = saturate_cast<int>(u * 32) on the double (half to even), then as above.
 *              fisheye: theta = atan(r), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
 *              scale = r == 0 ? 1 : theta_d / r, map = (fx x' scale + cx, fy y' scale + cy) (K without skew). */
#define RELOC_REMAP_INTER_BITS   5    /* 32 sub-pixel steps per axis, 1024 alphas */

/* RESIZE: cv2.resize(src, dsize, fx, fy, INTER_NEAREST | INTER_LINEAR | INTER_AREA) on 8-bit images (nearest also 16-bit, one
 * channel), restated from OpenCV 4.x modules/imgproc/src/resize.cpp (the reference: cv2.resize(img, (808, 616),
 * interpolation=cv2.INTER_AREA) between undistort and CLAHE, datasets/nclt/scripts/run_orbslam3_tuning.py:209-211,
 * run_all_visual_slam.py:182-183,217-218; not pinned against a cv2 build).  cvRound: half to even; cvFloor,
 * cvCeil on doubles; ss / ds = source / destination extent of an axis.
 *   sizes      dsize given: inv_scale = (double)ds / ss; dsize empty: ds = cvRound(ss * f) (saturating, >= 1 or an error),
 *              inv_scale = f as the caller gave it; scale = 1.0 / inv_scale.
 *   nearest    sx = min(cvFloor(dx * scale_x), sw - 1), the same in y.
 *   area_fast  iscale = cvRound(scale); area_fast = |scale_x - iscale_x| < DBL_EPSILON && |scale_y - iscale_y| < DBL_EPSILON.
 *              INTER_LINEAR with area_fast and iscale (2, 2) is computed as INTER_AREA.
 *   area       downscale on both axes only (scale >= 1).  area_fast: box = iscale_x x iscale_y source pixels from
 *              (dx iscale_x, dy iscale_y); wholly inside the source: (a + b + c + d + 2) >> 2 for (2, 2), otherwise
 *              saturate_cast<uchar>(sum * (1.f / (iscale_x iscale_y))), int sum, one f32 multiply; sticking out (fx / fy sizes
 *              only, (2, 2) included): saturate_cast<uchar>((float)sum / count) over the pixels inside; starting outside: 0.
 *              General: per axis and destination index d a tap list in double with f32 alphas: f1 = d scale, f2 = f1 + scale,
 *              cell = min(scale, ss - f1), s1 = cvCeil(f1), s2 = min(cvFloor(f2), ss - 1), s1 = min(s1, s2); taps
 *              (s1 - 1, (s1 - f1) / cell) if s1 - f1 > 1e-3, (s, 1 / cell) for s in s1 .. s2 - 1,
 *              (s2, min(min(f2 - s2, 1), cell) / cell) if f2 - s2 > 1e-3.  f32 without FMA: per y-tap (sy, beta) in order
 *              buf = 0.f + sum over x-taps in order of S[sy][sx] * alpha; acc = beta * buf for the first, acc += beta * buf
 *              after; dst = saturate_cast<uchar>(acc).  Channels independent.
 *   linear     f = (float)((dx + 0.5) * scale_x - 0.5), sx = cvFloor(f), f -= sx; sx < 0: sx = 0, f = 0; sx >= sw - 1:
 *              sx = sw - 1, f = 0; a0 = cvRound((1.f - f) * 2048), a1 = cvRound(f * 2048);
 *              H = S[sx] * a0 + S[min(sx + 1, sw - 1)] * a1.  Vertically the same f and sy but not zeroed at the edges, rows
 *              clip(sy, 0, sh - 1) and clip(sy + 1, 0, sh - 1), weights b0, b1;
 *              dst = (((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2.
 *   The library builds the per-axis tables on the host in exactly these words; the kernels do integer or f32 arithmetic on
 *   table entries only.  Everything else (other interpolations, dtypes, INTER_AREA upscaling) is refused. */
#define RELOC_RESIZE_LINEAR_BITS 11   /* INTER_RESIZE_COEF_BITS: the two weights of an axis sum to 2048 */

/* BAYER: cv2.cvtColor(raw, COLOR_Bayer??2BGR | COLOR_Bayer??2RGB) on 8-bit single-channel mosaics of at least 3 x 3, restated
 * from OpenCV 4.x modules/imgproc/src/demosaicing.cpp (bilinear Bayer2RGB_; the reference: cv2.cvtColor(raw,
 * cv2.COLOR_BayerGR2BGR) in front of undistort and BGR2GRAY, datasets/robotcar/scripts/prepare_stereo_euroc.py:43-45,117-137;
 * not pinned against a cv2 build).
 *   pattern    the two letters of a code are the colours of pixels (row 1, col 1) and (row 1, col 2); the top-left 2 x 2 tile:
 *              BG (46) = R G / G B (sensor name RGGB), GB (47) = G R / B G (GRBG), RG (48) = B G / G R (BGGR),
 *              GR (49) = G B / R G (GBRG).  The tile repeats over the image.
 *   interior   1 <= y <= h - 2, 1 <= x <= w - 2, integers on the raw bytes, N S W E NW NE SW SE the eight neighbours:
 *              red or blue site: own colour = raw, green = (N + S + W + E + 2) >> 2, opposite = (NW + NE + SW + SE + 2) >> 2;
 *              green site: green = raw, colour of the horizontal neighbours = (W + E + 1) >> 1, of the vertical ones
 *              (N + S + 1) >> 1.
 *   border     after the interior: column 0 copies column 1 and column w - 1 copies column w - 2 for rows 1 .. h - 2; then
 *              row 0 copies row 1 and row h - 1 copies row h - 2 over the whole width (so a corner takes the nearest interior
 *              pixel): dst(y, x) = interior(clamp(y, 1, h - 2), clamp(x, 1, w - 2)).
 *   2RGB       the same arithmetic with the output channels swapped; OpenCV's enum aliases: BayerBG2RGB = BayerRG2BGR,
 *              BayerGB2RGB = BayerGR2BGR, BayerRG2RGB = BayerBG2BGR, BayerGR2RGB = BayerGB2BGR.
 *   gray       the stage in front of ORB: the gray conversion above on the demosaiced (B, G, R), i.e. the bytes of
 *              cvtColor(cvtColor(raw, Bayer??2BGR), BGR2GRAY).  OpenCV's direct Bayer??2GRAY codes round differently (a 14-bit
 *              path of their own) and are refused, as are 16-bit mosaics and the _VNG, _EA and 2BGRA codes. */
#define RELOC_BAYER_BG2BGR       46
#define RELOC_BAYER_GB2BGR       47
#define RELOC_BAYER_RG2BGR       48
#define RELOC_BAYER_GR2BGR       49

/* PIXEL FORMATS: the packed 8-bit camera frames besides BGR / RGB, and cv2.cvtColor's conversions of them, restated from OpenCV
 * 4.x modules/imgproc/src/color_rgb.simd.hpp (RGB2Gray) and color_yuv.simd.hpp (YUV422toRGB8Invoker; not pinned against a cv2
 * build).  All integer.
 *   mono8      (H, W): the bytes are the gray.
 *   BGRA, RGBA (H, W, 4): COLOR_BGRA2GRAY (10) / COLOR_RGBA2GRAY (11) = the gray conversion at the head of this file on the
 *              first three channels, in the given order; the fourth byte is ignored.
 *   YUYV, UYVY (H, W, 2), W even: a pixel pair is the 4 bytes Y0 U Y1 V (YUYV = YUY2 = YUNV) or U Y0 V Y1 (UYVY = Y422 =
 *              UYNV).  YVYU (Y0 V Y1 U) has its Y bytes where YUYV has them.
 *     gray     COLOR_YUV2GRAY_YUY2 (124) / COLOR_YUV2GRAY_UYVY (123): the Y bytes, untouched (no range expansion).
 *     colour   COLOR_YUV2BGR_YUY2 (116), COLOR_YUV2BGR_UYVY (108) and the 2RGB twins (115, 107), BT.601 limited range:
 *              u = U - 128, v = V - 128, y = max(0, Y - 16) * CY, r = 1 << (SHIFT - 1);
 *              B = sat8((y + r + CUB * u) >> SHIFT), G = sat8((y + r + CVG * v + CUG * u) >> SHIFT),
 *              R = sat8((y + r + CVR * v) >> SHIFT); the shift is arithmetic (floor), sat8 clamps to 0..255, both pixels of a
 *              pair take the pair's U and V.  2RGB: the same values, R first.
 *   Planar 4:2:0 (NV12, I420), 16-bit mono, the 4-channel outputs and YVYU to colour are not implemented; the Y plane of a
 *   4:2:0 buffer, frame[:H], is a mono8 frame. */
#define RELOC_FMT_BGR            0    /* 3 interleaved bytes, BGR or RGB by the `order` argument: the default */
#define RELOC_FMT_MONO8          1
#define RELOC_FMT_BGRA           2
#define RELOC_FMT_RGBA           3
#define RELOC_FMT_YUYV           4
#define RELOC_FMT_UYVY           5
#define RELOC_YUV_SHIFT          20   /* ITUR_BT_601_SHIFT */
#define RELOC_YUV_CY             1220542
#define RELOC_YUV_CUB            2116026
#define RELOC_YUV_CUG            (-409993)
#define RELOC_YUV_CVG            (-852492)
#define RELOC_YUV_CVR            1673527

/* ORB MASK: cv2.ORB.detectAndCompute(image, mask) with an 8-bit single-channel mask of the image's size, restated from OpenCV
 * 4.x modules/features2d/src/orb.cpp (the mask pyramid of detectAndCompute, computeKeyPoints) and fast.cpp /
 * KeyPointsFilter::runByPixelsMask (not pinned against a cv2 build).
 *   pyramid    mask level 0 is the mask as given.  For l >= 1, mask level l = threshold(resize(mask level l - 1, size of
 *              level l, INTER_LINEAR_EXACT), RELOC_ORB_MASK_THRESH, 0, THRESH_TOZERO): the resize tables and arithmetic of
 *              the image pyramid above, then every value <= 254 becomes 0 -- a pixel survives only where the interpolation
 *              gives 255.  Level l is resized from the THRESHOLDED level l - 1 and level 1 from the raw mask, so a mask of
 *              values 0 / 1 keeps level 0 only (OpenCV's behaviour, kept).
 *   per level  FAST and the 3x3 non-maximum suppression run unmasked: the mask does not change which pixel is a local
 *              maximum.  A kept corner at the integer level pixel (x, y) is dropped iff mask level l at (y, x) is 0.  Then the
 *              edge margin, the score histogram, retainBest(2 x quota) with ties, Harris, best-quota, orientation and the
 *              descriptor exactly as without a mask (a dropped corner frees its place in the quota, which a filter behind
 *              ORB cannot do).  A level whose mask is non-zero everywhere is that of the unmasked detector. */
#define RELOC_ORB_MASK_THRESH    254  /* THRESH_TOZERO: values above it are kept */

/* ORB PARAMS: cv2.ORB_create(nfeatures, scaleFactor, nlevels, ..., scoreType, ..., fastThreshold) as runtime settings, restated
 * from OpenCV 4.x modules/features2d/src/orb.cpp (detectAndCompute, computeKeyPoints; not pinned against a cv2 build,
 * DESIGN.md section 2).  The constants at the head of this file are the defaults and RELOC_ORB_NLEVELS stays the capacity of
 * every per-level array.  edgeThreshold, patchSize, firstLevel and WTA_K are not settings.
 *   levels     scale of level l = (float)pow(scale_factor, (double)l) with scale_factor a double (OpenCV's Python binding
 *              rounds scaleFactor to float first; this restatement does not), level size = lrintf(w / scale) x lrintf(h / scale):
 *              today's expressions, so (8, 1.2) is today's pyramid bit for bit.
 *   quotas     factor = (float)(1.0 / scale_factor); n = (float)(nfeatures * (1 - factor) / (1 - (float)pow((double)factor,
 *              (double)nlevels))); level l < nlevels - 1 gets lrintf(n), then n *= factor; level nlevels - 1 gets
 *              max(nfeatures - sum, 0).
 *   unused     levels l >= nlevels are empty: w = h = stride = 0, quota 0; so is a level one of whose sizes rounds to 0 (its
 *              quota is spent on nothing).  A level takes keypoints iff w > 62 && h > 62 && quota > 0.
 *   FAST       segment test and score with the given threshold t: score = best - 1 if best > t, else 0 (no corner).
 *   stage 1    retainBest(n_keep) by FAST score with ties kept; n_keep = 2 * quota for HARRIS_SCORE, quota for FAST_SCORE.
 *              A level with no more than n_keep corners keeps all: its cut is t.  The RELOC_ORB_STAGE1_CAP raise as before.
 *   score      HARRIS_SCORE: Harris response of the stage-1 survivors, best quota with ties.  FAST_SCORE: no Harris pass, the
 *              response is (float)score and every stage-1 survivor is a keypoint, so ties at the cut make a level exceed
 *              its quota.  Output level-major, raster order inside a level; the excess over a context's rows is cut off.
 *   mask       between NMS and the histogram as before, on the mask pyramid of the same level geometry. */
#define RELOC_ORB_HARRIS_SCORE     0
#define RELOC_ORB_FAST_SCORE       1
#define RELOC_ORB_NLEVELS_MIN      1            /* .. RELOC_ORB_NLEVELS */
#define RELOC_ORB_SCALE_MIN        1.01
#define RELOC_ORB_SCALE_MAX        2.0
#define RELOC_FAST_THRESHOLD_MIN   1            /* the score plane is 8-bit and 0 means "no corner" */
#define RELOC_FAST_THRESHOLD_MAX   254

/* MATCH POLICY: how a record's descriptors are paired with the current frame's.  RELOC_MATCH_CROSS (the default) is
 * BFMatcher(NORM_HAMMING, crossCheck=True).match(desc_t, desc_curr), the matcher of visual_landmark_matcher.py:211,327.
 * RELOC_MATCH_RATIO restates experiments/62_tight_detour_anchor_sanity/scripts/checkpoint_a_selftest.py:68-77 (knnMatch(desc_curr,
 * desc_t, k=2), Lowe test, gather, solvePnPRansac) and the score of simulation/isaac/scripts/_archive/anchor_localizer.py:82-90:
 *   sets       query = the current frame's descriptors (column c, 0 <= c < C); train = the rows of ONE record (row r, 0 <= r < n).
 *   neighbours per query c: nearest row = smallest Hamming distance, lowest row index on ties (d1); second nearest = the
 *              smallest remaining (distance, index) (d2).  This is reloc_match_knn2(current, record), idx and dist alike.
 *   test       c is a match iff n >= 2 and (double)d1 < ratio * (double)d2: strict, in double, one multiplication.  A record of
 *              fewer than two rows yields no match; two identical rows nearest to c (d1 == d2) yield none at any ratio <= 1.
 *   list       (queryIdx = c, trainIdx = nearest row, distance = d1), in queryIdx order.  Up to C entries.
 *   pairs      keypoints_3d_cam[trainIdx], pts_curr_2d[queryIdx]: the opposite orientation to the crossCheck list, whose
 *              queryIdx is the teach row.
 *   score      of a record in the whole-database search: the length of its list.
 *   ratio      a finite double in (0, 1].
 *   gates      unchanged and in the reference's order: a record of len(desc_t) < min_matches rows is no candidate and is given
 *              no PnP (S:64), a list shorter than min_matches neither (S:72); inliers, reprojection, consistency as before. */
#define RELOC_LOWE_RATIO           0.80         /* LOWE_RATIO, visual_landmark_matcher.py:66 ("kept for docs"), S:71 */

/* STEREO: depth at the ORB keypoints from the other eye of a rectified pair.  The matcher is this project's own (nothing here
 * is OpenCV's), stated in integers so that tests/stereo_ref.py restates it bit for bit.
 *   inputs     two 8-bit gray planes L, R of the working-frame size w x h, rectified so that a scene point lies on the same row
 *              in both at x_R = x_L - d, d >= 0; keypoints (x, y) in float32 level-0 coordinates; fx in pixels of the working
 *              frame; baseline_m > 0; min_disparity in 0..1024; num_disparities in 8..256; uniqueness in 0..50; lr_check 0/1.
 *              The window is fixed: R = RELOC_STEREO_R, a (2R + 1) x (2R + 1) patch.
 *   per keypoint, in this order; the first failing step sets status, leaves depth_mm = 0 and disparity = 0 and ends it:
 *   1 border   u = rint(x), v = rint(y), half to even in float32 (np.round, k_record).  status 1 unless R <= u < w - R and
 *              R <= v < h - R.
 *   2 range    D = { d : min_disparity <= d < min_disparity + num_disparities, u - d - R >= 0 }.  status 2 when |D| < 3.
 *   3 cost     C(d) = sum over j, i in -R..R of |L[v + j, u + i] - R[v + j, u - d + i]|, int32.
 *   4 edge     d* = argmin C, lowest d on ties.  status 3 when d* is the smallest or the largest member of D.
 *   5 unique   C2 = min C(d) over d in D with |d - d*| >= 2.  status 4 when such a d exists and
 *              C2 * (100 - uniqueness) <= C(d*) * 100.  A flat patch (all costs equal) fails at 4 or here and never passes.
 *   6 LR       if lr_check: xr = u - d*; D' = { d' : min_disparity <= d' < min_disparity + num_disparities, xr + d' + R < w };
 *              C'(d') = sum |R[v + j, xr + i] - L[v + j, xr + d' + i]|; d'* = argmin C', lowest on ties.  status 5 when
 *              |d'* - d*| > 1.
 *   7 subpixel a = C(d* - 1), b = C(d*), c = C(d* + 1), den = a + c - 2b in integers.  delta = 0 when den <= 0, else
 *              (float)(a - c) / (float)(2 * den): one float32 division of exactly representable integers.
 *              disparity = (float)d* + delta, one float32 addition.
 *   8 depth    z = fx * baseline_m / (double)disparity in float64, mm = rint(z * 1000.0).  status 6 when mm > 65535, else
 *              depth_mm = (uint16)mm and status 0.
 * The result is what a depth camera would have delivered at that pixel: uint16 millimetres, 0 = no depth.  From there the
 * recorder's and the accumulation's arithmetic applies unchanged ((float)mm / 1000.0f, range gates, back-projection, lens
 * model).  The recorder's 3 x 3 depth-variance gate has no meaning for a per-keypoint depth and does not apply (sd = 0):
 * uniqueness and the left-right check take its place as the guard against depth discontinuities.
 *
 * STEREO, dense: the depth image of the pair.  For every integer pixel (u, v) of the working frame, steps 1 to 8 with x = u,
 * y = v (step 1 rounds nothing); no new parameter, no new status.  Three planes of the working-frame size w x h, w, h >= 2R + 1:
 *   depth_mm   uint16, 0 = no depth;   disparity  float32, 0 where status is not 0;   status  uint8, the seven codes below.
 * The plane at (rint x, rint y) is, by construction, what the per-keypoint form returns for keypoint (x, y).
 *   cost volume  all seven statuses can be read off one left-referenced volume C(v, u, d) = sum over j, i in -R..R of
 *              |L[v + j, u + i] - R[v + j, u - d + i]|, defined for R <= v < h - R, R <= u < w - R, d in D(u).  The search of
 *              step 6 from pixel (u, v) with xr = u - d* is C'(d') = C(v, xr + d', d'): the same absolute differences, summed
 *              over the same window.  So with the row's right disparity map dR(v, xr) = argmin over d' of C(v, xr + d', d'),
 *              lowest d' on ties, over min_disparity <= d' < min_disparity + num_disparities with xr + d' + R < w, step 6
 *              is |dR(v, u - d*) - d*| > 1.  The members of that search are exactly the defined entries of the volume on the
 *              diagonal u - d = xr (xr >= R holds wherever step 6 is reached), those of pixels that fail step 2 included.
 * A depth image made this way serves everything that takes one: the obstacle cloud (every step-th pixel, 0.3 to 10 m), the
 * depth-image form of the recorder with its 3 x 3 variance gate, a log.
 *
 * STEREO, speckle: an optional stage behind steps 1 to 8 of the dense pass, OpenCV's filterSpeckles as StereoBM / StereoSGBM
 * apply it (speckleWindowSize, speckleRange).  Two settings: speckle_window, the component size limit in pixels, 0 = off
 * (the default); speckle_range in whole disparities, 0..RELOC_STEREO_SPECKLE_RANGE_MAX, default 1.
 *   filter     filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on a 2-D int16 plane: a pixel is valid when it differs
 *              from newVal; two 4-neighbours are joined when both are valid and |a - b| <= maxDiff, the difference taken in
 *              int32; a component is a connected component of that relation (transitive through chains, never diagonal);
 *              every pixel of a component of at most maxSpeckleSize pixels becomes newVal, nothing else changes.  OpenCV
 *              states it as a raster-order flood fill; the result does not depend on the order.
 *   quantise   q = (int16)rint(disparity * 16.0f) where status is 0 (the product is exact, rint rounds half to even; every
 *              such q is positive), q = -16 elsewhere -- status 6 included.
 *   stage      the filter with newVal = -16, maxSpeckleSize = speckle_window, maxDiff = 16 * speckle_range.  A pixel of
 *              status 0 that it removes gets status 7, depth_mm 0 and disparity 0; no other pixel changes.
 * tests/speckle_ref.py restates filter and stage.
 *
 * STEREO, semi-global: an optional aggregation between the cost volume and the selection of the dense pass.  This is the
 * recurrence of semi-global matching over this project's SAD costs, not OpenCV's StereoSGBM (no Birchfield-Tomasi cost, no
 * 5-direction mode, no disparity scaling).
 *   volume     C(v, u, d) of "STEREO, dense", defined for R <= v < h - R, R <= u < w - R and d in D(u) = { min_disparity <= d <
 *              min_disparity + num_disparities, u - d - R >= 0 }.  A pixel is in the domain when it lies in those row and
 *              column bounds and D(u) is not empty.
 *   settings   path_mask in 1..255, bit b selects direction r_b = (du, dv): 0 (+1, 0), 1 (-1, 0), 2 (0, +1), 3 (0, -1),
 *              4 (+1, +1), 5 (-1, -1), 6 (+1, -1), 7 (-1, +1); paths = 4 is mask 0x0F, paths = 8 mask 0xFF.
 *              0 <= P1 <= P2 <= RELOC_STEREO_SGM_P2_MAX; the defaults are 8 and 32 times the 121 pixels of the window.
 *   path cost  for a selected direction r, a domain pixel p = (u, v), its predecessor q = p - r and d in D(p):
 *              L_r(p, d) = C(p, d) when q is not in the domain; else, with m = min over k in D(q) of L_r(q, k),
 *              L_r(p, d) = C(p, d) + min( L_r(q, d), L_r(q, d - 1) + P1, L_r(q, d + 1) + P1, m + P2 ) - m,
 *              a term whose disparity is not in D(q) left out (m + P2 always exists).  C <= 30855 and L_r <= C + P2 < 2^16.
 *   sum        S(p, d) = sum of L_r(p, d) over the selected directions, below 2^19.
 *   selection  steps 2 and 4 to 8 of "STEREO" with S in place of C: d* = argmin S, lowest d on ties; the edge gate; the
 *              uniqueness gate on S; the left-right gate with dR(v, xr) = argmin over d' of S(v, xr + d', d'), lowest d' on
 *              ties, over the defined entries of that diagonal; the parabola through S(d* - 1), S(d*), S(d* + 1) (integers
 *              below 2^22, exact in float32); the depth.  The same eight status codes and three planes; the speckle stage
 *              behind it is unchanged.
 *   identity   with P1 = P2 = 0 every L_r equals C, so S = n C for n selected directions: the argmin, both gates (a common
 *              factor on both sides) and the parabola's quotient (numerator and denominator scaled alike, and the division
 *              is correctly rounded) are those of C, and every plane equals the dense pass bit for bit, for every mask.
 * tests/stereo_sgm_ref.py restates it.
 *
 * STEREO, census: an optional data term for pairs whose eyes are exposed unequally (own auto-exposure and gain per camera,
 * vignetting per lens).  One setting, cost: RELOC_STEREO_COST_SAD (0, the default: everything above) or
 * RELOC_STEREO_COST_CENSUS (1).
 *   transform  T(I) of a w x h 8-bit plane I, w, h >= 1, is a w x h 8-bit plane: bit k of T(I)[v, u] is set when
 *              I[clamp(v + dj_k, 0, h - 1), clamp(u + di_k, 0, w - 1)] < I[v, u].  The comparison is strict: equal values give
 *              0.  (di_k, dj_k), k = 0..7, is (-2,-2) (0,-2) (2,-2) (-2,0) (2,0) (-2,2) (0,2) (2,2), di along the row.
 *              Coordinates are clamped to the image, not to the stride: no byte outside 0 <= x < w, 0 <= y < h is read.
 *   cost       with the census, step 3 reads C(d) = sum over j, i in -R..R of popcount(T(L)[v + j, u + i] xor
 *              T(R)[v + j, u - d + i]), and step 6's C' is formed likewise.  0 <= C <= 8 * 121 = 968.
 *   unchanged  steps 1, 2 and 4 to 8, the statuses, the dense identity C'(d') = C(v, xr + d', d'), the speckle stage and the
 *              semi-global recurrence, which runs over these costs as it runs over the SADs.  A flat window (every T equal,
 *              a constant gray value among them) has all costs 0 and fails at step 4 or 5 as before.
 *   invariance T(a I + b) = T(I) for a > 0 wherever nothing clips and no two compared values round onto each other: the
 *              transform keeps the order of gray values and nothing else, so an eye that is re-exposed costs what it cost.
 *   penalties  the semi-global defaults over census costs are one and four bits on each of the window's 121 pixels,
 *              RELOC_STEREO_SGM_P1_CENSUS_DEFAULT and _P2_CENSUS_DEFAULT; the SAD defaults over costs of at most 968
 *              over-smooth.  A setting's own defaults (reloc_set_stereo_sgm with paths 0) stay the SAD ones.
 * tests/stereo_census_ref.py restates it. */
#define RELOC_STEREO_COST_SAD          0
#define RELOC_STEREO_COST_CENSUS       1
#define RELOC_STEREO_SGM_P1_CENSUS_DEFAULT 121  /* 1 * 121 */
#define RELOC_STEREO_SGM_P2_CENSUS_DEFAULT 484  /* 4 * 121 */
#define RELOC_STEREO_R                 5
#define RELOC_STEREO_MIN_DISPARITY_MAX 1024
#define RELOC_STEREO_NUM_DISP_MIN      8
#define RELOC_STEREO_NUM_DISP_MAX      256
#define RELOC_STEREO_NUM_DISP_DEFAULT  128
#define RELOC_STEREO_UNIQUENESS_MAX    50
#define RELOC_STEREO_UNIQUENESS_DEFAULT 15
#define RELOC_STEREO_OK          0
#define RELOC_STEREO_BORDER      1
#define RELOC_STEREO_RANGE       2
#define RELOC_STEREO_EDGE        3
#define RELOC_STEREO_UNIQUENESS  4
#define RELOC_STEREO_LR          5
#define RELOC_STEREO_FAR         6
#define RELOC_STEREO_SPECKLE     7
#define RELOC_STEREO_SPECKLE_RANGE_MAX 255
#define RELOC_STEREO_SGM_P1_DEFAULT    968      /* 8 * 121 */
#define RELOC_STEREO_SGM_P2_DEFAULT    3872     /* 32 * 121 */
#define RELOC_STEREO_SGM_P2_MAX        8191

/* OCCUPANCY: the teach-time occupancy map of the reference's teach_run_depth_mapper.py (D below): a 2-D log-odds grid that
 * the obstacle cloud of a frame is ray-traced into, written as .pgm + .yaml for the repeat run's static costmap layer.
 * Restated in tests/occupancy_ref.py, which the library equals cell for cell.  D line by line except (g).
 *   (a) cloud    (N, 3) float32 points in a sensor frame, in a fixed order; rows with a non-finite coordinate are dropped
 *              (D:60).  The depth-image form produces exactly the cloud of reloc_depth_points: every step-th pixel,
 *              zmin < z < zmax, finite, point = (z, -px, -py), raster order.
 *   (b) map      T: the 3 x 4 sensor-to-map transform, float64, row major (D's _tf_to_matrix, computed by the host).
 *              x = ((T00 * px + T01 * py) + T02 * pz) + T03, likewise y and z: float64, this order, no FMA contraction.
 *   (c) filter   keep z_lo < z < z_hi in float64 (D: 0.2, 2.0).  Among the points kept by (a) and (c) together, in input order,
 *              the rays are those of rank 0, s, 2s, ...; s = subsample (D: 4).
 *   (d) cells    col = trunc((x - origin_x) / res), row = trunc((y - origin_y) / res) in float64, toward zero like Python's
 *              int() (D:120-123): a coordinate in (origin - res, origin) lands in cell 0.  In-grid is decided on the double
 *              (-1 < q < W), before any integer conversion.  The start cell comes from (T03, T13); if it is outside the
 *              grid the frame marks nothing.
 *   (e) rays     for every ray whose end cell is in the grid, D's Bresenham (D:172-195; err = dr - dc, both conditional
 *              steps): every cell before the end cell gets a free update, the end cell a hit.  A ray whose end cell is
 *              outside the grid marks nothing.  A zero-length ray is a hit on the start cell.
 *   (f) units    D's log-odds are multiples of 0.2; the grid holds integers in units of 0.2: free -2, hit +7, bounds -25 and
 *              +25.  Classes of the .pgm: occupied (0) iff units >= 4 (D: > ln(0.65 / 0.35) = 0.619), free (254) iff
 *              units <= -6 (D: < ln(1 / 3) = -1.0986), unknown (205) otherwise; rows flipped (D's np.flipud).
 *   (g) frame    THE DEVIATION.  D clamps after every single update, which makes a cell depend on the order of the updates
 *              it receives within a frame.  Here a cell gets one update per frame:
 *              v = clamp(v + 7 * hits - 2 * frees, -25, +25).  The two agree on every cell that receives only frees or only
 *              hits within a frame; they can differ only where a cell receives both kinds in one frame and a bound engages.
 *   (h) counters frames_skipped_empty: the cloud of (a) is empty.  Nothing moves when (c) leaves nothing or the start cell is
 *              outside the grid.  Otherwise frames_integrated += 1 and total_points_integrated += number of rays, those
 *              dropped in (e) included. */
#define RELOC_OCC_L_FREE       (-2)
#define RELOC_OCC_L_OCC        7
#define RELOC_OCC_L_MIN        (-25)
#define RELOC_OCC_L_MAX        25
#define RELOC_OCC_UNITS_OCC    4      /* units >= this: occupied */
#define RELOC_OCC_UNITS_FREE   (-6)   /* units <= this: free     */
#define RELOC_OCC_PGM_OCC      0
#define RELOC_OCC_PGM_FREE     254
#define RELOC_OCC_PGM_UNKNOWN  205
#define RELOC_OCC_MAX_CELLS    (1 << 24)   /* capacity of one grid: w_cells * h_cells */
#define RELOC_OCC_SUBSAMPLE_DEFAULT 4

/* CORRELATION: the depth-correlation anchor of the reference's depth_correlation_matcher.py (C below): the cells of the current
 * depth cloud are slid over the dilated teach occupancy map and the offset with the most hits becomes an anchor.  Restated in
 * tests/correlation_ref.py, which the library equals in every integer it returns.  C line by line.
 *   (a) map      the .pgm plane with rows flipped (C:84-85), occupied = (pixel == 0) (C:86), row 0 at origin_y.  Dilated n
 *              times (C:89-90, iterations = dilate_cells, C's default 1) by SciPy's DEFAULT structuring element: the
 *              4-connected cross, whatever C's comment says of a 3 x 3 square.  One iteration: a cell is occupied iff it or one
 *              of its four edge neighbours was; cells beyond the border count as empty.  n = 0: the plane as it is.
 *   (b) cloud    OCCUPANCY (a): rows with a non-finite coordinate are dropped first (C:108).  No row left: status
 *              NO_DEPTH_POINTS (C:170-172).
 *   (c) map pt   OCCUPANCY (b) with the 3 x 4 float64 sensor-to-map transform, same operations, same order (C:175-179; the
 *              host composes the transform).
 *   (d) filters  keep z_lo < z < z_hi, both strict (C:183; 0.2, 2.0), and dx * dx + dy * dy < R * R with dx = x - vio_x,
 *              dy = y - vio_y: float64, each operation rounded, no contraction, R * R computed once (C:184-185's
 *              hypot(dx, dy) < MAX_RANGE, 15.0).  (vio_x, vio_y) is the BASE position, not the sensor's.  Fewer than
 *              min_points (C: 100) points kept: status TOO_FEW_POINTS, the record's kept count is what C logs (C:187-189).
 *   (e) cells    OCCUPANCY (d) for col from x and row from y (C:192-194): truncation toward zero, in the map iff
 *              0 <= cell < n after truncation.  Fewer than min_points POINTS (not cells) in the map: status OUT_OF_BOUNDS,
 *              the in-map count is what C logs (C:196-198).
 *   (f) scan     the set of distinct (row, col) of the points in the map; n_cells its size (C:200-201).
 *   (g) search   offsets (i, j), i, j in [-ns, ns], ns = int(window / step) (C:135-139).  The cell offset of index k is
 *              t[k + ns] = int(round(k * step / res)) with Python's round (C:210-211); the host computes this table of
 *              2 ns + 1 entries and hands it over.  i shifts columns, j rows.  hits(i, j) = number of scan cells (r, c) with
 *              (r + t[j], c + t[i]) inside the map and occupied there (C:212-219).  Entries may repeat.
 *   (h) best     scores in i-major, j-minor order; best = the first strictly greater than every score before it, starting
 *              from 0 hits at (i, j) = (0, 0) (C:204-223): an all-zero surface gives (0, 0) with 0 hits.  second = the second
 *              element of the scores sorted descending (C:226-228): equal to best when the maximum is tied, 0 for a table of
 *              one entry.
 *   (i) host     float64, C's expressions: frac = hits / n_cells (0.0 when n_cells == 0), peak_ratio = hits / max(1, second)
 *              (C:225-229); gates in this order: hits < min_hits -> low_hits, frac < min_fraction -> low_fraction, peak_ratio <
 *              min_peak_ratio -> not_significant, hypot(dx, dy) > consistency_m -> consistency_fail_{:.1f} (C:231-248) with
 *              dx = i * step, dy = j * step; anchor = (vio_x + dx, vio_y + dy, base z, base quaternion) (C:251-272);
 *              std = min(0.10 + 0.15 / max(1.0, peak_ratio - 1.0), 0.25), covariance [0] = [7] = std * std, [14] = 0.25,
 *              [21] = [28] = [35] = 0.05 (C:255-261); outcome published_std{:.2f}_shift{:.2f}; the CSV header and row of
 *              C:132, 152-156.
 * The record of a tick: RELOC_CORR_RECORD_WORDS int32: status, kept points (d), points in the map (e), n_cells, best i, best j,
 * best hits, second hits; the two point counts are always the frame's, behind a status other than OK the last five words are 0
 * and so is the whole surface. */
#define RELOC_CORR_OK               0
#define RELOC_CORR_NO_DEPTH_POINTS  1
#define RELOC_CORR_TOO_FEW_POINTS   2
#define RELOC_CORR_OUT_OF_BOUNDS    3
#define RELOC_CORR_RECORD_WORDS     8
#define RELOC_CORR_MAX_CELLS   (1 << 24)   /* capacity of one map: w * h ... */
#define RELOC_CORR_MAX_SIDE    32768       /* ... and cells per side */
#define RELOC_CORR_MAX_DILATE  64          /* iterations of (a) */
#define RELOC_CORR_MAX_TABLE   255         /* entries of the offset table (g): 2 ns + 1 */
#define RELOC_CORR_MAX_OFFSET  32768       /* magnitude of one entry, cells */
#define RELOC_CORR_MAX_WINDOW  703         /* side of the scan's window, cells: 2 * (ceil(max_range / res) + 2) + 1 */
#define RELOC_CORR_MIN_POINTS_DEFAULT 100

/* ROUTE: route clearance, what the reference does to keep a route's waypoints out of obstacles: offline sanitize_route.py (S
 * below, the same file in experiments 58..64) on the teach map, live send_goals_hybrid.py (H below; _project_wp and costmap_cb,
 * H:200-262) on every costmap update.  Both walk a grid breadth first; here the walk's depth is a distance plane and the walk's
 * order a table.  Restated in tests/route_ref.py, which the library equals in every byte and index it returns.
 *   (a) grid     a plane is h x w, row 0 at origin_y.  The cell of a point: col = int((x - origin_x) / res), row likewise from y,
 *              float64, truncation toward zero as Python's int() (S:78-79, H:114-115): a point up to one cell left of the map
 *              lands in column 0.  Not floor.  Always computed on the host.
 *   (b) occupied two sources: a host uint8 plane, non-zero = occupied (S.load_teach_map: flipud(img) == 0), or the context's
 *              occupancy grid where it lies, occupied iff units >= RELOC_OCC_UNITS_OCC: the cells reloc_occ_read's pgm paints 0.
 *   (c) stamps   a list of cell rectangles [r_lo, r_hi) x [c_lo, c_hi), OR-ed into the occupied plane on the device before (d);
 *              the part of a rectangle outside the plane is dropped.  The host computes them with S.stamp_obstacles'
 *              arithmetic (S:55-72): a cone is the one cell of (a), dropped when off the map; the tent is clipped as S clips it.
 *   (d) clearance uint8: the L1 (city-block) distance in cells to the nearest occupied cell where that is <= cap, else
 *              RELOC_ROUTE_FAR; cap in [0, RELOC_ROUTE_MAX_CAP]; a plane with no occupied cell is all RELOC_ROUTE_FAR.  S's walk
 *              (S:75-96) steps to 4-neighbours inside the rectangle and does not stop at obstacles, so its depth IS the L1
 *              distance; its `d > max_cells` test lets distance max_cells itself count.
 *   (e) re-entry S.find_safe_shift hands a candidate cell's corner origin_x + c * res back to dist_to_nearest_occupied
 *              (S:118-121), which recomputes the cell as int(((origin_x + c * res) - origin_x) / res): in float64 sometimes
 *              c - 1.  The same for rows.  The host computes both int32 tables once per map with exactly that expression; the
 *              device reads the clearance of a candidate at [row_remap[r]][col_remap[c]].  The waypoint's own first test (S:164)
 *              uses no remap.
 *   (f) order    an order table: the (dr, dc) in the order the reference's walk dequeues them from a start cell, neighbours
 *              up, down, left, right = (-1, 0), (1, 0), (0, -1), (0, 1), layer by layer through layer m.  H enqueues off-map
 *              cells (H:227-232): its table is always the unclipped diamond, 2 m (m + 1) + 1 entries, 1861 at m = 30.  S enqueues
 *              only in-map cells (S:125-129): its table is the walk clipped to min(r0, m), min(h - 1 - r0, m), min(c0, m),
 *              min(w - 1 - c0, m) cells around the start.  The clipped table is the unclipped one without its off-map entries,
 *              in the same order: every cell that enqueues an in-map cell lies between it and the start, hence in the map as
 *              well, so layer by layer the in-map cells keep the order they have among all cells (tests/test_route_host.py
 *              holds the two equal for every clip).  (g) skips off-map cells, so the unclipped table serves S and H alike,
 *              and a whole route is one search.  The host runs the walk on an empty window and hands the table over: the
 *              queue defines the order.
 *   (g) search   one order table, n start cells: for each start the smallest table index k whose cell (r0 + dr_k, c0 + dc_k) is
 *              inside the plane and satisfies the predicate; -1 when there is none.
 *   (h) predicates CLEARANCE: clearance[row_remap[r]][col_remap[c]] >= d_min.  COST: 0 <= cost[r][c] < thresh on an int8
 *              costmap; negative (unknown) and off-map cells are blocked (H:124-131).
 *   (i) thresholds d_min: the smallest integer d with d * res >= safety_m in float64, found on the host by trying d = 0, 1, ...;
 *              the comparison S itself makes (S:121, 165), not a quotient: 17 * 0.1 = 1.7000000000000002 >= 1.7 holds through
 *              the product's rounding.  The plane's cap is
 *              ceil(safety_m / res) + 2 (S:109, 121).  The host asserts d_min <= int(safety_m / res) + 2, the cap of S:164: one
 *              plane then answers both of S's calls, since only `>= d_min` is ever asked of it. */
#define RELOC_ROUTE_FAR             255       /* clearance: no occupied cell within cap */
#define RELOC_ROUTE_MAX_CAP         254
#define RELOC_ROUTE_MAX_SIDE        32768     /* cells per side of a map or costmap; cells in all: RELOC_OCC_MAX_CELLS */
#define RELOC_ROUTE_MAX_OFFSETS     65536     /* entries of one order table: m = 180 layers unclipped */
#define RELOC_ROUTE_MAX_OFFSET      32767     /* magnitude of one entry's dr or dc, cells */
#define RELOC_ROUTE_PRED_CLEARANCE  0
#define RELOC_ROUTE_PRED_COST       1

/* OBSTACLE: local obstacle perception, what the reference's repeat driver asks of every depth frame: traversability_filter.py (F
 * below), gap_navigator.py's depth_to_obstacle_profile (N below) and local_obstacle_grid.py (G below; the files of experiment
 * 39 and scripts/_archive).  Restated in tests/obstacle_ref.py, which the library equals bit for bit in everything but the
 * variance of (d), where the decision is the rule.
 *   (a) pixel    z in metres is the one depth pixel of the teach path: float32 as it is, uint16 as f32(mm) / 1000.0f.  Valid iff
 *              z > lo && z < hi and z is finite; lo, hi float32 with 0 <= lo, the bounds themselves invalid (F:36-38, N:69-73,
 *              G:97-101).
 *   (b) strip    rows [h / 3, 2 h / 3) in integer division (N:63-64, G:86-88); columns 0, step, 2 step, ... with step >= 1
 *              (N:67 step 1, G:95 step 4).
 *   (c) percentile of a column's n valid values, sorted ascending as s, equal to np.percentile(valid_float32, q) (N:75, G:106):
 *              qf = f32(q) / f32(100), vi = f32(n - 1) * qf, lo_i = floor(vi), hi_i = min(lo_i + 1, n - 1), g = vi - f32(lo_i),
 *              d = s[hi_i] - s[lo_i]; the result is s[hi_i] - d * (1 - g) if g >= 0.5f, else s[lo_i] + d * g.  float32, every
 *              operation rounded on its own, no contraction.  q an integer percent in [0, 100].  A column with n < min_valid
 *              yields the caller's fill (N:74 needs n >= 4, G:103 n >= 3); the count n is returned beside it.  A strip of more
 *              than RELOC_OBS_MAX_STRIP rows is beyond the capacity.
 *   (d) traversability (F:21-53) over the (h / bh) x (w / bw) whole blocks; remainder rows and columns are never touched.  Per
 *              block over the pixels valid under (a) with F's own lo, hi (0.3, 10.0): the count n, the minimum, and the variance
 *              in float64 in two passes (mean, then mean of squared deviations).  Traversable iff n >= min_count (F:40, 10),
 *              n <= n_cov with n_cov the largest n for which n / (bh * bw) < coverage in float64 (F:43, 49; the host finds it,
 *              the device compares integers), variance > var_thresh (F:48) and (double)min > min_solid (F:50).  Every pixel of a
 *              traversable block reads as fill (F:51, 10.0) for whatever comes behind.  The device sums in a fixed tree, numpy's
 *              float32 np.var pairwise: the value may differ in its last bits, so a fixture keeps every block's variance more
 *              than 1e-3 relative away from the threshold.
 *   (e) grid     cells x cells float32, the robot at centre = cells / 2 (G:22-25).  One update, in G's order (G:42-122):
 *              shift by (sx, sy) whole cells with zero fill, new[r][c] = old[r + sy][c + sx] or 0 outside (G:57-70: np.roll by
 *              -sx on axis 1, then by -sy on axis 0; |s| >= cells clears everything); every cell times f32(decay) (G:76); then,
 *              with a depth source, for the columns of (b) in ascending order whose n >= min_valid: depth = (double)percentile,
 *              gx = centre + (int)(depth * c / res), gy = centre + (int)(depth * s / res) in float64, truncated toward zero
 *              (G:108-113), (c, s) that column's entry of a direction table the host computes (G:90-92, 108: cos and sin of
 *              yaw + linspace(-fov / 2, fov / 2, w)[col]); if (gx, gy) is inside the grid, f32(hit) is added to it and f32(hit_nb)
 *              to (gx + 1, gy), (gx - 1, gy), (gx, gy + 1), (gx, gy - 1), each only if inside (G:115-122).  The additions to a
 *              cell are float32 and happen in exactly that order: 0.45f is not exact, so the order is part of the answer.  The
 *              host computes sx = int((x - prev_x) / res), sy likewise (G:50-55), prev updated on every frame (G:72-73).
 *   (f) sectors  (G:124-157) one direction-table entry per sector; dist starts at 2 * res and grows by dist += res in float64
 *              while dist < max_range; the cell is (centre + (int)(dist * c / res), centre + (int)(dist * s / res)); leaving
 *              the grid ends the ray with max_range, the first cell with value >= obstacle_hits ends it with dist.  float64 out.
 *   (g) read-out the grid; G's debug image (uint8)(clip(grid / hits, 0, 1) * 255) in float32 (G:159-162); the number of cells
 *              >= obstacle_hits and the maximum (G:164-168). */
#define RELOC_OBS_MAX_STRIP      512       /* rows of the strip (b) */
#define RELOC_OBS_MAX_COLS       4096      /* width of a depth image of these entry points */
#define RELOC_OBS_MIN_BLOCK      4         /* side of a block of (d) ... */
#define RELOC_OBS_MAX_BLOCK      64        /* ... */
#define RELOC_OBS_MAX_CELLS      512       /* cells per side of the grid (e) */
#define RELOC_OBS_MAX_GRID_COLS  1024      /* columns of (b) that one grid update projects */
#define RELOC_OBS_MAX_SECTORS    4096      /* sectors of one profile (f) */
#define RELOC_OBS_MAX_STEPS      (1 << 20) /* max_range / res of (f) */
#define RELOC_MORPH_MAX_KERNEL    4096      /* side of the rectangle of reloc_morph_rect; a pixel reads min(side, image side) pixels */
#define RELOC_MORPH_MAX_ITERATIONS 64

#endif /* RELOC_SPEC_H */
