/*
 * orbx_debug.h -- introspection of liborbx.so intermediate buffers (test use).
 * Copies one stage buffer of image `image` of the handle's last extraction to
 * host memory so the parity tests can localise a mismatch to a stage.
 */
#ifndef ORBX_DEBUG_H
#define ORBX_DEBUG_H
#include "orbx.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  ORBX_DBG_BLUR_LEVEL = 1,  /* arg = level: blurred level image (w*h bytes)                 */
  ORBX_DBG_CELL_COUNTS = 2, /* int32 per FAST cell (all levels, row-major per level)         */
  ORBX_DBG_CELL_TABLE = 3,  /* int32 x8 per cell: level,x0,y0,x1,y1,cand_off,cap,0           */
  ORBX_DBG_CANDIDATES = 4,  /* u32 per candidate slot (score<<24|y<<12|x), cand_total slots   */
  ORBX_DBG_OCT_COUNTS = 5,  /* int32 per level                                                */
  ORBX_DBG_OCT_OUT = 6,     /* u32 per octree output slot, oct_total slots                    */
  ORBX_DBG_LEVEL_INFO = 7,  /* int32 x8 per level: w,h,cell_begin,cell_end,oct_off,oct_cap,nfeat,nIni */
  ORBX_DBG_PATCH_SLOTS = 8  /* int32 x128: k_describe's patch slot s = lane + 64 * load -> row << 2 | chunk
                               of the row's span, 255 = unused (the table the kernel reads; no image)   */
};

/* Returns the number of bytes the item occupies (copies min(cap, size)); <0 on error. */
long long orbx_debug_copy(orbx_extractor* h, int what, int image, int arg, void* dst, size_t cap);

/* k_resize's launch descriptors and the block-remap constants for one image geometry, built on the
 * host exactly as an extractor handle builds them (no device is needed or touched).  Every item is a list of
 * int64 words; table pointers are reported as element offsets into their tables.  Returns the
 * number of words of the item (copies min(cap, words) of them to dst, which may be NULL); <0 on
 * error (ORBX_ERR_ARG, or the plan's ORBX_ERR_SIZE). */
enum {
  ORBX_LP_LEVELS = 1,     /* x8 per level: w, h, pyramid off, blurred off, bstride, tile_begin, tiles_x, tiles_y */
  ORBX_LP_RESIZE = 2,     /* x16 per level >= 1 (k_resize): sw, sh, dw, dh, src_off (-1: the input image),
                             dst_off, pyr_bytes, xtab_off, ytab_off, bx_off, by_off, stride, rows, lc,
                             tile columns, tile rows */
  ORBX_LP_BOUNDS = 3,     /* x2 per entry of the footprint-bound table bx_off / by_off index:
                             (sx0 of a tile column's first, sx1 of its last output column), resp. (sy0, sy1) */
  ORBX_LP_GRIDS = 4,      /* x3 per launch: the grids (gx, gy, gz) of k_resize for levels 1.. and of k_blur for a
                             batch of a0 images */
  ORBX_LP_REMAP = 5,      /* x8, the division-free block remap of a gx=a0, gy=a1, gz=a2 grid:
                             gx, gy, total >> 3, total & 7, magic x, shift x, magic y, shift y;
                             l / g == (((2l + 1) * magic) >> 32) >> shift for every l < gx*gy*gz */
  ORBX_LP_XTAB = 6,       /* x4 per output column of level a0 >= 1: sx0, sx1, a0, a1 (the resize coefficients) */
  ORBX_LP_YTAB = 7,       /* x4 per output row of level a0 >= 1: sy0, sy1, b0, b1 */
  ORBX_LP_PATH = 8,       /* x8 per level >= 1, the resize kernel chosen for it: path (1: k_resize_strip, 0: k_resize),
                             tile columns, tile rows (its grid), tile width, tile height, LDS row stride,
                             footprint rows staged, strip rows per thread (0 for k_resize) */
  ORBX_LP_FAST = 9,       /* x8 per k_fast launch group: first cell, end cell, then the kernel instance k_fast<S, RP, NK>
                             (LDS row stride, region rows per compass instruction, window loads per lane) and
                             its LDS: window tile bytes, score map bytes, bytes per block */
  ORBX_LP_OCTREE = 10,    /* x8 per k_octree launch group, the groups of a batch of three or more images first, then
                             the one launch of smaller batches: first level, end level, threads per block, LDS node
                             capacity, largest cell count of a level, kcap (a level's candidates kept in LDS; the
                             rest go through global scratch), dynamic LDS bytes, the largest batch that takes this
                             row (-1 for the groups: every larger batch) */
  ORBX_LP_CELLS = 11,     /* x8 per FAST cell: level, x0, y0, x1, y1 (the detection region, inclusive), the cell's
                             offset in ORBX_DBG_CANDIDATES' logical view (as ORBX_DBG_CELL_TABLE), cap (its
                             candidate slots), kin (those of them that are inline) */
  ORBX_LP_OCT_LEVELS = 12,/* x8 per level, DistributeOctTree's inputs and outputs: minBorderX, minBorderY, maxBorderX,
                             maxBorderY, N (the level's quota), nIni (clamped to 1), the level's offset in
                             ORBX_DBG_OCT_OUT, its output slots */
  ORBX_LP_OCT_PYRAMID = 13/* x8 per k_octree launch group, ORBX_LP_OCTREE's rows in its order: the count pyramid's
                             depth D (0: the group's blocks run the generic path only), the root count it is
                             sized for (the largest nIni of the group's levels), its 16-bit counters (depths
                             0..D, depth 0 padded to an even count) and their bytes, the pyramid path's LDS
                             bytes, the generic path's, the dynamic LDS of the launch (the larger of the
                             two), the largest depth the plan considers */
};
long long orbx_debug_launch_plan(const orbx_extractor_params* params, int width, int height, int what, int a0,
                                 int a1, int a2, long long* dst, size_t cap);

/* The shipped stereo matcher (orbx_stereo_match's launch path, unchanged) on keypoints and
 * descriptors the caller supplies instead of the extractions' own (tests only: scenes that place a
 * keypoint on every boundary of Frame::ComputeStereoMatches).  Preconditions as orbx_stereo_match
 * without the fingerprint check: both handles' last call was orbx_extract, on the same geometry and
 * device (ORBX_ERR_STATE / ORBX_ERR_ARG otherwise); the matcher reads their device pyramids.  The
 * supplied arrays go to a scratch block of this call, so the handles' extraction state is untouched
 * and a later orbx_stereo_match on the true outputs still succeeds.
 * Outputs (nL each): uRight and depth after the median filter; sad, the per-keypoint SAD the match
 * kernel left (-1 unless accepted before the filter); *nmatches, the matches the filter kept.
 * Checked on the host before any device call: ORBX_ERR_CAPACITY for nR > 4096; ORBX_ERR_ARG unless
 * every keypoint passes orbx_debug_stereo_keypoints_check on the handles' geometry. */
orbx_status orbx_debug_stereo_keypoints(orbx_extractor* left, orbx_extractor* right, const orbx_keypoint* kpsL,
                                        const uint8_t* descL, int nL, const orbx_keypoint* kpsR, const uint8_t* descR,
                                        int nR, float bf, float baseline, float* uRight, float* depth, int32_t* sad,
                                        int32_t* nmatches);
/* ORBX_OK when every keypoint has octave in [0, nlevels) and finite x, y in [0, width) x [0, height)
 * without a sign bit (-0.0f is refused: the matcher sorts on y's bit pattern); ORBX_ERR_ARG
 * otherwise.  The matcher indexes its level and row tables with these unguarded.  No device is
 * needed or touched. */
int orbx_debug_stereo_keypoints_check(const orbx_keypoint* kps, int n, int nlevels, int width, int height);

/* The shipped k_octree (orbx_extract's launch path for a batch of n_img images, unchanged: one launch
 * over every level for one or two images, the launch groups beyond) on FAST candidates the caller
 * supplies instead of k_fast's own (tests only: scenes that drive DistributeOctTree down every path).
 * Precondition: the handle's last call was an extraction (ORBX_ERR_STATE otherwise); its geometry and
 * device are used.  Per image: cell_counts, one int32 per FAST cell (ORBX_DBG_CELL_COUNTS' layout), and
 * candidates in ORBX_DBG_CANDIDATES' logical view (score << 24 | y << 12 | x in level coordinates,
 * every cell's cap slots from its ORBX_LP_CELLS offset on, its first count slots read).  They go to a
 * scratch block of this call in the kernel's inline / overflow slot layout, so the handle's
 * extraction state is untouched.  Outputs per image: oct_count (nlevels values, ORBX_DBG_OCT_COUNTS)
 * and oct_out (ORBX_DBG_OCT_OUT's slots, filled with 0xFFFFFFFF before the launch, so a slot the
 * kernel did not write shows).  Checked on the host before any device call: ORBX_ERR_ARG unless the
 * input passes orbx_debug_octree_candidates_check on the handle's geometry. */
orbx_status orbx_debug_octree_candidates(orbx_extractor* h, int n_img, const int32_t* cell_counts,
                                         const uint32_t* candidates, int32_t* oct_count, uint32_t* oct_out);
/* The same launch, which also reports per (image, level), n_img x nlevels values, the path the level's
 * block took: 0 an empty level, 1 the count-pyramid path, 2 the generic path (ORBX_LP_OCT_PYRAMID; a
 * block leaves the pyramid path when a round selects a node of depth D that holds several candidates,
 * or when the level holds more than 65535).  The kernel writes the path through a pointer that is null
 * in every other launch.  depth_cap >= 0 runs the launch groups at min(D, depth_cap) with the plan's
 * LDS (0: the generic path alone, as a plan whose D is 0 runs); -1 leaves the plan's D. */
orbx_status orbx_debug_octree_paths(orbx_extractor* h, int n_img, const int32_t* cell_counts,
                                    const uint32_t* candidates, int depth_cap, int32_t* oct_count,
                                    uint32_t* oct_out, int32_t* paths);
/* ORBX_OK when n_img is in [1, 64], every cell's count is in [0, cap], every candidate read has x in
 * [minBorderX, maxBorderX) and y in [minBorderY, maxBorderY) of its cell's level, and no two
 * candidates of one level of one image share a pixel; ORBX_ERR_ARG otherwise (also for a geometry
 * without a FAST cell), or the plan's ORBX_ERR_SIZE.  The kernel subtracts the minimum border and packs
 * 12-bit fields unguarded, and its best-response pass relies on FAST's one candidate per pixel.  The
 * plan is built on the host as orbx_debug_launch_plan builds it: no device is needed or touched. */
int orbx_debug_octree_candidates_check(const orbx_extractor_params* params, int width, int height, int n_img,
                                       const int32_t* cell_counts, const uint32_t* candidates);

/* The library's deterministic double atan2 (Sim3Solver's half-angle, src/Sim3Solver.cc:325) evaluated
 * on the host: the same operation sequence as the kernels run (no device is needed or touched). */
double orbx_debug_atan2_det(double y, double x);

/* The Levenberg step every LM kernel of the library runs (OptimizationAlgorithmLevenberg::solve), compiled
 * for the host: no device is needed or touched.  state = lambda, ni, currentChi, iniChi, rho and
 * counts = qmax, nBad are updated in place.  ops bit 0: one trial's verdict on (tempChi, scale = the sum
 * x_j (lambda x_j + b_j), ok2 = the solve succeeded) with the cube of cube_kind (0: the plain product
 * x*x*x of PoseOptimization, OptimizeSim3 and OptimizeEssentialGraph; 1: LocalBundleAdjustment's cube
 * rounded once, std::pow(x, 3)).  ops bit 1: then the iteration-end rule.  Returns bit 0 = accepted,
 * bit 1 = another trial follows, bit 2 = the phase terminates; ORBX_ERR_ARG (-1) for a null pointer, a
 * cube_kind other than 0 / 1 or ops outside 1..3. */
int orbx_debug_lm_step(double state[5], int counts[2], double tempChi, double scale, int ok2, int cube_kind,
                       int ops);

/* The library's deterministic double exp (g2o::Sim3's std::exp(sigma)) of n values, on the device. */
int orbx_debug_exp(const double* x, int n, double* y, int device);
/* VertexSim3Expmap::oplusImpl on the device, in a one-thread kernel: out = Sim3(update) * S with
 * update[6] zeroed first when fix_scale; S and out are eight doubles as orbx_optimize_sim3_problem.S12. */
int orbx_debug_sim3_exp(const double update[7], const double S[8], int fix_scale, double out[8], int device);

/* The library's deterministic double log / acos (g2o::Sim3::log's std::log(s) and acos(d)) of n values,
 * on the device. */
int orbx_debug_log(const double* x, int n, double* y, int device);
int orbx_debug_acos(const double* x, int n, double* y, int device);
/* g2o::Sim3::log() of n Sim3 (eight doubles each) on the device: out n x 7 (omega, upsilon, sigma);
 * branch (optional, n): bit 0 = d <= 1 - eps, bit 1 = |sigma| >= eps, bits 2 and 3 = a row exchange at
 * the first / second pivot of W.lu(). */
int orbx_debug_sim3_log(const double* S, int n, double* out, int32_t* branch, int device);
/* Optimizer::OptimizeEssentialGraph's first linearisation (the problem's points and outputs are not
 * read): per edge the measurement (8), the error (7) and both numeric Jacobians (7 x 7 row-major, rows =
 * error entries; zero for the fixed vertex), then the assembled system at the initial estimates: H dense
 * N x N (N = 7 (n_vertices - 1), both triangles) and b (N).  Any output may be NULL. */
int orbx_debug_essgraph_linearize(const orbx_essential_graph_problem* problem, double* meas, double* err,
                                  double* J0, double* J1, double* H, double* b, int device);
/* One solve (H + lambda I) x = b through the envelope LDL^T of the problem's graph (only its structure
 * is read): H dense N x N whose non-zeros lie in that envelope (its lower triangle is read).  *ok = 0 on
 * a zero pivot (x is then not meaningful). */
int orbx_debug_essgraph_solve(const orbx_essential_graph_problem* problem, const double* H, const double* b,
                              double lambda, double* x, int32_t* ok, int device);
/* orbx_optimize_essential_graph with the Levenberg kernel's own phase times (its 100 MHz wall clock,
 * summed over the run): phase_ms[0] linearise + assemble, [1] factor + substitute, [2] the rest of the
 * trials (update, errors, chi2, control); *envelope_blocks (optional): 7 x 7 blocks of the envelope. */
int orbx_debug_essgraph_phases(const orbx_essential_graph_problem* problem, const orbx_essential_graph_result* result,
                               double phase_ms[3], long long* envelope_blocks, int device);

/* Solve S x = b (N x N, N a multiple of 6) with the LocalBA reduced-system
 * LDLT kernel; *ms = mean kernel time over reps launches.  ORBX_ERR_STATE on
 * a zero pivot. */
int orbx_debug_ldlt(const double* S, const double* b, int N, double* x, int reps, float* ms);
/* The same with the kernel chosen as orbx_ba_debug_options.ldlt does; stamps (optional, 64 words):
 * the kernel's s_memtime phase stamps of the last launch, when built with -DORBX_LDLT_TS.  N up to
 * 3072 for ORBX_BA_LDLT_TILED and ORBX_BA_LDLT_AUTO (*ms is then the whole launch sequence), a padded
 * size of 1024 for the others (ORBX_ERR_HIP beyond). */
int orbx_debug_ldlt_ex(const double* S, const double* b, int N, double* x, int reps, float* ms, int kind,
                       unsigned long long* stamps);

/* LocalBA test options of one solver handle (tests and tools only; a production caller never sets
 * them: ldlt = AUTO with nan_trial = raise_stop_after = -1 is the shipped behaviour).  ldlt forces
 * one of the reduced-system kernels the library ships for other sizes (so each is tested at every
 * size it can take); the two hooks reproduce rare events deterministically: nan_trial (the chi2 of
 * that trial of each phase reads NaN, the reference's rho-NaN rejection) and raise_stop_after (the
 * stop flag reads raised after that many trials). */
#define ORBX_BA_LDLT_AUTO 0    /* 8-wide panels (N < 128), column-step (N <= 192), blocked MFMA to 1024, tiled beyond */
#define ORBX_BA_LDLT_COLUMN 1  /* the column-step kernel wherever it fits */
#define ORBX_BA_LDLT_BLOCKED 2 /* the blocked MFMA kernel */
#define ORBX_BA_LDLT_TILED 3   /* the tiled kernels over many workgroups (AUTO: only beyond a padded size of 1024) */
typedef struct {
  int ldlt;             /* ORBX_BA_LDLT_* */
  int nan_trial;        /* -1 off */
  int raise_stop_after; /* -1 off */
  int trace;            /* one timing line per call on stderr */
  int fused_ctl;        /* 1: a trial's errors and LM verdict in ONE launch (k_ba_errors_ctl: the
                           partials handed to the last block through a release/acquire ticket)
                           instead of the shipped two (k_ba_errors + k_ba_lm_control); tests
                           compare them bit for bit */
} orbx_ba_debug_options;
/* NULL restores the defaults. */
int orbx_debug_ba_options(orbx_ba* h, const orbx_ba_debug_options* options);

/* Capture of one LM trial's linear algebra (tests only; off by default, and while off the solver
 * launches nothing for it).  orbx_debug_ba_capture_select arms the handle for its next orbx_ba_run /
 * orbx_ba_run_bool (the selection holds for that one run; orbx_ba_run_many does not capture): the first
 * trial of phase `phase` (0: the robust optimize(5), 1: optimize(10) on the inliers) whose iteration
 * index within the phase is `it` (-1: any) and whose trial index within its iteration is `q` (the value
 * LmState::qmax has when the trial starts).  (0,0,0) is phase 1's entry trial, (0,1,0) its first
 * relinearised trial, (1,0,0) phase 2's entry trial, (p,-1,1) the first retry of phase p.  phase < 0
 * disarms.  The run's results are bit-identical with and without a capture.
 *
 * orbx_debug_ba_capture_read copies item `what` of the last capture to dst and returns the item's size
 * in bytes (copies min(cap, size)); ORBX_ERR_STATE when no capture fired (HEADER is always readable
 * and says so), ORBX_ERR_ARG otherwise.  Items are double unless marked int32.  Sizes: nc cameras, np
 * points, ne edges of the problem; na active edges (positions), npa active points, nposes free
 * cameras with an active edge in the captured phase; N = 6 * nposes.
 *
 * Two states are recorded.  The CURRENT state (CQ, CT, X) is what the device held when the trial's
 * solve began: the state EERR was computed at.  The LINEARISED state is what the trial's step is applied
 * to: CBAK / XBAK for the free poses / active points, the current state elsewhere.  They are equal on a
 * q = 0 trial; on a retry the current state is still the rejected estimate (k_ba_update pops it), and
 * EERR are that estimate's errors, as g2o keeps them. */
enum {
  ORBX_BA_CAP_HEADER = 0,     /* int32 x12: fired, phase, it, q, solve ok, trial index within the phase,
                                 nc, np, ne, na, npa, nposes                                            */
  ORBX_BA_CAP_LAMBDA_CHI = 1, /* x2: lambda the trial used, LmState::currentChi at its start            */
  ORBX_BA_CAP_CQ = 2,         /* nc x4: current rotation quaternions (x, y, z, w)                       */
  ORBX_BA_CAP_CT = 3,         /* nc x3: current translations                                            */
  ORBX_BA_CAP_X = 4,          /* np x3: current points                                                  */
  ORBX_BA_CAP_EERR = 5,       /* ne x3: stored edge errors (row 2 of a mono edge is 0; edges outside ACT
                                 keep whatever an earlier phase left)                                   */
  ORBX_BA_CAP_S = 6,          /* N x N row-major: k_ba_schur_fin's reduced matrix before the LDLT touches
                                 it; every entry is defined (both triangles are written)                */
  ORBX_BA_CAP_BS = 7,         /* N: its right-hand side                                                  */
  ORBX_BA_CAP_XP = 8,         /* N: the solve's pose step (zero when the solve failed, also the next three) */
  ORBX_BA_CAP_CBAK = 9,       /* nposes x7: q (x, y, z, w), t of pose i's camera before the trial's update */
  ORBX_BA_CAP_XBAK = 10,      /* npa x3: active point i before the update                               */
  ORBX_BA_CAP_XL = 11,        /* npa x3: the point step, X after the update minus XBAK                  */
  ORBX_BA_CAP_ACT = 12,       /* int32 na: active edge ids in position order (point-major)              */
  ORBX_BA_CAP_POSE_CAM = 13,  /* int32 nposes: Hessian pose index -> camera                             */
  ORBX_BA_CAP_PT_ID = 14,     /* int32 npa: active point index -> point                                 */
  ORBX_BA_CAP_EROBUST = 15    /* int32 ne: 1 where the edge carries its Huber kernel                    */
};
int orbx_debug_ba_capture_select(orbx_ba* h, int phase, int it, int q);
long long orbx_debug_ba_capture_read(orbx_ba* h, int what, void* dst, size_t cap);

/* On-box HBM reference: copy `bytes` (multiple of 16) between two device
 * buffers with a streaming 16-B kernel, reps times on the null stream;
 * *ms = mean time per copy (2 * bytes of HBM traffic each). */
int orbx_debug_hbm_copy(void* dst, const void* src, size_t bytes, int reps, float* ms);

/* orbx_initializer_create + orbx_initializer_initialize with the kernels' own routines compiled for
 * the host and run there stage by stage (no device is touched): the CPU half of the parity tests,
 * which pins the arithmetic against the literal restatement before anything runs on a GPU. */
int orbx_debug_initializer_host(const float* keys1_xy, int n1, const float K[9], float sigma, int iterations,
                                const float* keys2_xy, int n2, const int32_t* matches12, const int32_t* rand_vals,
                                int n_rand, int* used, float R21[9], float t21[3], float* p3d,
                                uint8_t* triangulated, orbx_initializer_result* result);
float orbx_debug_acosf_det(float x);

/* CreateNewMapPoints test options of one handle (a production caller never sets them; NULL restores
 * the defaults).  raise_after_neighbour: the stop flag reads raised at every check after that
 * neighbour's loop body (-1 off), as LocalBA's raise_stop_after.  probes: the next host calls also
 * bring back the per-pair and per-neighbour intermediates below (off: they cost nothing). */
typedef struct {
  int raise_after_neighbour;
  int probes;
} orbx_new_points_debug_options;
int orbx_debug_new_points_options(orbx_new_points* h, const orbx_new_points_debug_options* options);
/* The probes of the handle's last host call, n_neighbours rows each; returns the item's size in bytes
 * (copies min(cap, size)), ORBX_ERR_STATE when that call ran without probes. */
enum {
  ORBX_NP_PROBE_EXIT = 0,    /* uint8 x n1 per neighbour: ORBX_NP_* of feature idx1's pair */
  ORBX_NP_PROBE_COS = 1,     /* float x n1 x 3: cosParallaxRays, cosParallaxStereo1, cosParallaxStereo2 */
  ORBX_NP_PROBE_F12 = 2,     /* float x 9 (zero for a neighbour the gate skipped) */
  ORBX_NP_PROBE_MATCH12 = 3  /* int32 x n1: the search's match12 (-1 everywhere for a neighbour that did not run) */
};
long long orbx_debug_new_points_probe(orbx_new_points* h, int what, void* dst, size_t cap);
/* Neighbour `neighbour`'s share of CreateNewMapPoints with the kernels' own routines compiled for the
 * host (no device is touched): the gate (skip code, baseline, median depth, F12) and, when it ran, the
 * per-pair routine on the caller's match12 (n1 entries, -1 none).  Per feature of the current keyframe:
 * exit (n1), cos (n1 x 3), pos / normal (n1 x 3), dist (n1 x 2); values are written where exit is an
 * accepted code.  The caller owns the chain (has_mp between neighbours) and the search. */
int orbx_debug_new_points_host(const orbx_new_points_problem* problem, int neighbour, const int32_t* match12,
                               int32_t* skip, float* baseline, float* median_depth, float F12[9], uint8_t* exit_code,
                               float* cos3, float* pos, float* normal, float* dist);

#ifdef __cplusplus
}
#endif
#endif
