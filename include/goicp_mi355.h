/* goicp_mi355.h -- C ABI of libgoicp_mi355.so, the MI355X-native (gfx950, HIP) Go-ICP engine.
 *
 * Drop-in boundary for the hot path of zjsun1017/CUDA-Go-ICP: BnB cube-bound evaluation, the
 * inner ICP loop and the rotation-cube search.  Every entry point names the reference interface
 * it replaces (paths relative to the reference checkout).  Plain pointers and sizes only; all
 * matrices are row-major float[9]; clouds are packed float xyz triples.
 *
 * Conventions
 *   - every function returns GOICP_OK (0) or a negative goicp_status; the message of the last
 *     failure on the calling thread is available from goicp_last_error().
 *   - handles are opaque; one handle per host thread, except goicp_poll()/goicp_cancel(), which
 *     are safe concurrently with goicp_register() (the reference's viewer polls the worker,
 *     src/goicp_kernel.cu:161-177).
 *   - output buffers are caller-owned unless a matching *_free() exists.
 *   - there is NO CPU fallback: goicp_create() fails with GOICP_ERR_NO_DEVICE without a GPU.
 *   - numerical contract: per-point arithmetic is bit-identical to the reference CPU path
 *     (src/goicp/); sums are tree reductions, so bounds agree to ~1e-5 relative.
 */
#ifndef GOICP_MI355_H
#define GOICP_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOICP_ABI_VERSION 4

typedef enum goicp_status {
	GOICP_OK = 0,
	GOICP_ERR_INVALID = -1,    /* bad argument */
	GOICP_ERR_IO = -2,         /* file missing / unreadable / malformed  (reference: std::runtime_error, src/common.cpp:139-142,196-199,210,226) */
	GOICP_ERR_CONFIG = -3,     /* TOML parse error / missing info.description (src/common.cpp:28-40) */
	GOICP_ERR_NO_DEVICE = -4,  /* no HIP device: the product never computes on the CPU */
	GOICP_ERR_DEVICE = -5,     /* HIP runtime failure (reference: exit(EXIT_FAILURE), src/kernel.cu:29-38) */
	GOICP_ERR_INTERNAL = -6,
	GOICP_ERR_TIMEOUT = -7,    /* a collective of the sharded search did not complete within the communicator's deadline: the
	                              process must exit non-zero (a rank is lost); never re-execute */
	GOICP_ERR_PEER = -8        /* another rank of the sharded search reported a failure (goicp_shard_stats.failed_rank) */
} goicp_status;

const char* goicp_last_error(void);
int goicp_abi_version(void);
/* first 16 hex digits of the SHA-256 over the kernel sources (csrc/device.hip, bnbqueue.hip, kdbuild.hip, device.hpp, in that order)
 * this library was built from -- measurement hygiene: counter profiles under profiles/ carry the hash they were collected on */
const char* goicp_kernel_source_hash(void);

/* ---------------------------------------------------------------------------------------------
 * Config  -- replaces class Config (src/common.h:133-180, src/common.cpp:12-77).
 * Same keys, defaults and clamps.  Keys the reference declares but never parses
 * ([params.rotation], [params.translation], search_depth: src/common.h:157-169) are read here too.
 * ------------------------------------------------------------------------------------------- */
#define GOICP_PATH_MAX 1024
typedef struct goicp_config {
	int32_t mode;                 /* 0 ICP CPU, 1 ICP GPU, 2 ICP k-d tree GPU, 3 Go-ICP CPU, 4 Go-ICP GPU (src/common.h:7-11) */
	int32_t trim;
	float subsample;              /* clamped to [0,1]      (src/common.cpp:63) */
	float mse_threshold;          /* clamped to >= 1e-10   (src/common.cpp:64) */
	float resize;
	char target[GOICP_PATH_MAX];
	char source[GOICP_PATH_MAX];
	char output[GOICP_PATH_MAX];
	char visualization[GOICP_PATH_MAX];
	float viz_theta, viz_phi;
	int32_t viz_spin_after_finish;
	float rot_min[3], rot_max[3];     /* degrees */
	int32_t rot_search_depth;
	float trans_min[3], trans_max[3];
	int32_t trans_search_depth;
	char description[GOICP_PATH_MAX];
	int32_t has_rotation_range;       /* the TOML carries a [params.rotation] table (test/skull_goicp.toml:22-30) */
	int32_t has_translation_range;    /* ... a [params.translation] table (test/skull_goicp.toml:32-41) */
} goicp_config;

int goicp_config_load(const char* toml_path, goicp_config* out);

/* ---------------------------------------------------------------------------------------------
 * Cloud loader -- replaces load_cloud / load_cloud_ply / load_cloud_txt (src/common.cpp:79-228):
 * ".ply" (ascii or binary_little_endian, element vertex with float x,y,z, other properties and
 * elements skipped) or ".txt" ("N" then N lines "x y z").  Points are multiplied by `resize`;
 * `subsample` keeps each point with that probability, capped at floor(N*subsample).
 * seed = 0 reproduces the reference's non-deterministic std::random_device seeding.
 * ------------------------------------------------------------------------------------------- */
int goicp_cloud_load(const char* path, float subsample, float resize, uint64_t seed, float** xyz, size_t* n);
void goicp_cloud_free(float* xyz);

/* ---------------------------------------------------------------------------------------------
 * Engine -- replaces icp::FastGoICP + icp::Registration + icp::IterativeClosestPoint3D
 * (src/fgoicp/fgoicp.hpp:11-69, registration.hpp:44-98, icp3d.hpp:9-41) with the CPU path's
 * semantics (GoICP, src/goicp/jly_goicp.h:84-142).
 * ------------------------------------------------------------------------------------------- */
typedef struct goicp_engine* goicp_handle;

typedef struct goicp_params {
	int32_t dt_size;         /* DT grid side, reference 300 (src/goicp/jly_goicp.cpp:56) */
	double dt_expand;        /* bbox expand factor, reference 2.0 (src/goicp/jly_goicp.cpp:57) */
	float mse_threshold;     /* SSE threshold = mse_threshold * N (src/goicp/jly_goicp.cpp:208, src/fgoicp/fgoicp.hpp:23) */
	int32_t dt_layout;       /* 0 linear [z][y][x]; 1 bricked 4x4x4 (default) */
	int32_t device;          /* HIP device ordinal, -1 = current */
	int32_t trans_batch;     /* translation nodes expanded per search per launch; 1 = reference visit order */
	int32_t wide_children;   /* 1: the rotation children's ub and lb inner searches run in lock-step; 0 = reference order */
	int32_t icp_max_iter;    /* reference 10000 (src/goicp/jly_icp3d.hpp:114) */
	int32_t verbose;
	int32_t morton_sort;     /* source order on the device: 0 input order, 1 Morton curve, 2 k-d order (default) */
	int32_t rot_batch;       /* most rotation nodes expanded per round when wide_children (default 64; rounds ramp 8, 16, 32 ...) */
	int32_t kd_gpu_build;    /* k-d tree (box hierarchy) built on the device (Morton order, looser boxes): 1 yes, 0 or -1 host median splits (default) */
	float trim_fraction;     /* GoICP::trimFraction (src/goicp/jly_goicp.h:116): fraction of the largest residuals ignored; reference 0 */
	/* Search domain: the [params.rotation] / [params.translation] tables of the reference's configs
	 * (test/skull_goicp.toml:22-41; declared in src/common.h:157-169 but never parsed or applied there).
	 * use_* = 0 (default): the CPU path's fixed domain (src/goicp/jly_goicp.cpp:44-53), rotation cube [-pi,pi]^3 in
	 * angle-axis space, translation cube [-0.5,0.5]^3, unlimited depth.  use_* = 1: the root cube is the smallest cube
	 * that contains the box, children outside the box are never evaluated as candidates or expanded; a rotation range
	 * of +-180 degrees on every axis is the reference root itself.  *_search_depth > 0: nodes at that depth are
	 * evaluated but not split further (the guarantee is then limited to that resolution). */
	int32_t use_rot_range, use_trans_range;
	float rot_min[3], rot_max[3];       /* degrees; components of the angle-axis vector */
	float trans_min[3], trans_max[3];   /* in cloud units after `resize` */
	int32_t rot_search_depth, trans_search_depth;
	int32_t icp_fused;       /* 1: one launch per ICP iteration, the last workgroup to arrive runs the update;
	                          * 0: correspondence pass + update as two launches (same per-point arithmetic; the sums are added in
	                          * another order, so the states agree within float rounding -- not to the bit by construction) */
	int32_t bounds_fp16;     /* 1: the BnB cube bounds read a half-precision copy of the bricked DT (one 128-byte line per 4x4x4 brick
	                          * instead of two), rounded toward zero so that lower bounds stay valid.  Each LOOKED-UP VALUE comes out
	                          * low by < 2^-10 relative where its half is normal (2^-14 .. 65504 in cloud units; below that by
	                          * < 2^-24 absolute, above it the value is 65504); a bound deviates by more than that, because the
	                          * rotation radius subtracted from the value (v - rho) amplifies the relative error of what is left.
	                          * ICP, the DT re-score of a pose and trimmed bounds keep the fp32 grid.  No effect with dt_layout = 0:
	                          * the copy is made of the bricked grid only, and a linear-layout engine evaluates fp32 bounds.  NOT the
	                          * bit-parity path: opt-in, default 0 */
	int32_t icp_nn_cache;    /* opt-in (default 0; measured slower on real ICP trajectories).  1: the ICP pass keeps, per source point, its last neighbour m, the position q_ref it was found at
	                          * and a lower bound s on the distance from q_ref to every OTHER target point (a 2-nearest walk); at a later
	                          * position q the walk is skipped whenever |q - m| + |q - q_ref| < s, which proves m is still THE nearest
	                          * neighbour -- exact, not approximate; 0: every query walks the tree in every pass (bit-identical results) */
	int32_t flow;            /* opt-in (default 0 = lock-step batches: every rotation batch runs until its slowest inner search has stopped).
	                          * L > 0: continuous flow of the outer search over the device queues -- a rotation child is handled as soon as
	                          * both its inner searches have stopped, and the next rotation parents are admitted when at most L searches
	                          * still run.  Same bounds and prune rules, same optimum; more speculative work -- faster or slower depending
	                          * on which candidate happens to be refined first */
	int32_t adaptive_k;      /* 1 (default): when few inner searches are still running (the stragglers of a batch) each may expand up to 512
	                          * nodes per round instead of trans_batch: fewer latency-bound rounds; 0: always trans_batch */
	int32_t queue_cap;       /* test hook: nodes a device-resident queue may hold before its batch is re-run through the host queues
	                          * (0 = the full 8 192-node slab) */
	int32_t device_queues;   /* 1 (default): the inner-BnB translation queues live on the device -- a round of all active inner
	                          * searches is two launches, no host round trip; 0: host-side queues (always used with trans_batch == 1,
	                          * the reference visit order) */
	int32_t lds_tiles;       /* LDS-staged distance-transform tiles (north_star (a)) for the device-queue search: an inner search whose
	                          * selected nodes lie within tile_spread_vox voxels of each other (the deep rounds of a search) has them
	                          * evaluated by bounds_tile_kernel -- the DT box a 64-point patch of the cloud can reach under ALL of them is
	                          * staged in LDS once, a lookup is a ds_read -- instead of by the gathering kernel; same per-point float
	                          * expressions (bounds agree to the order of the sums).  2 (default): that evaluation is launched only while the
	                          * previous rounds had searches that qualify (shallow registrations never pay for it); 1: every round; 0: off */
	float tile_spread_vox;   /* default 10 */
	int32_t tile_min;        /* fewest expansions of a search for the tile list (default and minimum 8) */
	int32_t stale_widen;     /* adaptive_k refinement (default 1).  An inner search whose incumbent did not improve in its last round is PROVING, not finding: every
	                          * queued node whose lower bound is more than SSEThresh below the incumbent has to be expanded whatever the order (the per-node
	                          * stop rule, jly_goicp.cpp:257, admits nothing else), so a wider round wastes no cube bound and saves rounds.  1: its round
	                          * doubles after one such round and again after three; 2: x4 after one; 0: off */
	int32_t ub_tiebreak;     /* opt-in (default 0: measured, no registration got faster -- ties are rare beyond level 2).  1 (widened search only): rotation cubes of EQUAL lower bound and width are
	                          * expanded in the order of the smallest upper bound their own inner search saw (the basin most likely to refine the
	                          * optimum first).  The reference leaves that order to its heap (src/goicp/jly_goicp.h:44-56); any order of a best-first
	                          * BnB keeps the bounds valid.  0: the reference's key only.  Ignored in the reference-order mode */
	int32_t icp_point_seed;  /* 1 (default): every neighbour walk of the ICP pass / NN operator starts from a REAL candidate -- per DT voxel the engine keeps the
	                          * leaf slot of a target point whose seed voxel is nearest (the exact EDT passes once more, carrying their arg-min; V^3 x 4
	                          * bytes, built with the k-d tree) -- instead of from the distance-transform bound |q - c(v)| + DT[v] + 0.9 voxel, whose slack
	                          * leaves far-from-surface queries a shell of dozens of candidate leaves.  Exactness does not depend on the table (any
	                          * target point is a valid candidate; ties still go to the lowest index).  0: the DT bound */
	float ub_share;          /* widened search: on top of the rot_batch parents drawn by smallest lower bound, this fraction more are drawn per batch by the
	                          * smallest upper bound seen inside them (needs ub_tiebreak = 1; default 0 = none: measured slower) */
	int32_t twin_fusion;     /* 1 (default): the two inner searches of a rotation child -- GoICP::InnerBnB without and with the rotation uncertainty
	                          * (jly_goicp.cpp:494 and :532), same rotated cloud -- run in lock-step; when both list the SAME translation node in a
	                          * round its 8 children are gathered from the distance transform ONCE and the two passes' sums are formed from the
	                          * same fetched values (bit-identical to separate evaluations).  0: every listed node is evaluated on its own */
	int32_t sort_items;      /* 1 (default): a round of >= 2 048 expansions (the first rounds of a rotation batch: hundreds of rotations x whole levels of
	                          * the translation tree) walks its (expansion, 4 096-point chunk) work items in the order of the distance-transform cell
	                          * their gathers land in, so that an XCD's L2 serves neighbouring items instead of streaming the grid from the Infinity
	                          * Cache.  Changes no bound's terms, only the chunking of its sum.  0: search order */
	int32_t stale_compact;   /* default 2048.  A proving inner search (stale_widen) whose queue holds at least this many nodes selects its next nodes by
	                          * the Morton order of their corners instead of by lower bound: every queued node that passes the stop rule
	                          * (jly_goicp.cpp:257) has to be expanded whatever the order, a run of Morton-neighbours is spatially compact (LDS-tile
	                          * material) and is explored depth-first-like, so the queue slab stops overflowing into the host fall-back.  0: always
	                          * by lower bound (the reference's order, jly_goicp.h:64-71) */
	/* (icp_nn_cache, above: 2 = the exact neighbour cache switched on in the tail of a run only -- round 4, measured +0..3 %, opt-in) */
	int32_t stream_priority; /* 0 (default): the engine's HIP stream has the default priority; 1: the highest the device offers (hipStreamCreateWithPriority)
	                          * -- for a latency-bound engine (an ICP loop) that shares the GPU with a throughput engine; measured: tools/overlap_probe.py */
	int32_t lanes;           /* lanes of the device-queue search (round 4): a batch of at least lane_min_searches inner searches (GoICP::InnerBnB calls,
	                          * jly_goicp.cpp:227-340 -- independent of each other) is cut into lanes by rotation child and the lanes run their lock-step
	                          * rounds side by side on their own HIP streams, each with its own lists and control block, so one lane's dependent launches
	                          * drain beside the others'.  0 (default): three lanes when the previous batch's mean round was throughput-bound (>= 64 M
	                          * point-expansions: a count, so the choice is deterministic); 1: never; 2..4: that many, for every batch of at least
	                          * lane_min_searches.  Same searches, same bounds, same result per search; measured (tools/lanes_probe.py): prove-the-optimum
	                          * bunny 6.74 -> 5.7 s, synthetic 40 k 721 -> 649 ms, default (early-exit) registrations never qualify and are unchanged */
	int32_t lane_min_searches; /* default 64 */
	int32_t bounds_order;    /* tuning only.  goicp_eval_bounds_device on a bricked fp32 grid that fits the Infinity Cache: 0 the groups of eight cubes are walked as they
	                          * came; 1 a device pre-pass orders them by run of equal rotation (in arrival order) and, inside a run, by the Morton cell of the
	                          * parent cube's centre, so that the workgroups in flight gather from neighbouring distance-transform lines; 2 and two
	                          * neighbours of that order are evaluated by one workgroup, sharing the point load and the rotation.  Every cube's bounds are the same bits in all forms */
	int32_t bounds_order_min_groups; /* tuning only: batches of fewer groups keep the plain launch */
	int32_t bounds_order_max_runs;   /* tuning only: batches with more runs of equal rotation are walked as they came (at most 64) */
	float bounds_order_cell;         /* tuning only: smallest Morton cell of the order, in distance-transform voxels (<= 0: the default) */
	int32_t bounds_order_reprobe;    /* tuning only (default 64): once the pre-pass has left a batch alone, batches of the same size take the plain launch without a
	                                  * pre-pass, and every this-many-th of them runs it again; 0: every batch runs the pre-pass */
	int32_t bounds_balance;          /* default 1.  Form 2 over a cloud cut into eight point chunks: the eight block labels of the launch (blocks b and b + 8 share an
	                                  * XCD) take equal shares of the chunks' COST -- the distinct distance-transform lines a wavefront of the chunk gathers, counted on
	                                  * the device once per source cloud -- instead of one chunk each; 0: one chunk each.  Scheduling only: same bits either way */
	float bounds_balance_a;          /* tuning only: the weight of a wavefront against one line in that cost (<= 0: the default) */
	int32_t bounds_dedup;            /* default 1.  Form 2 over a cloud cut into several point chunks: an expansion that a run of equal rotation lists more than once --
	                                  * all eight cube records equal as raw bits, as the root expansion listed by every inner search of a rotation -- is evaluated
	                                  * once, and the other listings take its sums; 0: every listing is evaluated.  Same bits either way */
} goicp_params;

void goicp_params_default(goicp_params* p);
/* defaults + what a parsed config carries for the engine: mse_threshold and, when the TOML has them, the search
 * ranges and depths (main.cpp:33-42 reads mse_threshold the same way) */
void goicp_params_from_config(const goicp_config* c, goicp_params* p);

/* FastGoICP::FastGoICP(pct, pcs, mse_threshold, mtx) (src/fgoicp/fgoicp.hpp:14-28) + Registration ctor
 * (registration.hpp:66-80) + GoICP::BuildDT/Initialize (src/goicp/jly_goicp.cpp:75-90,134-209):
 * uploads both clouds, builds the distance transform (exact EDT, on the GPU) and the k-d tree. */
int goicp_create(const goicp_params* params, const float* target_xyz, size_t n_target,
                 const float* source_xyz, size_t n_source, goicp_handle* out);
int goicp_destroy(goicp_handle h);
/*
 * goicp_set_source: a new source cloud on a live handle (PCL's setInputSource under a fixed target).  Everything derived from the target
 * is kept -- the distance transform and its fp16 copy, the k-d hierarchy, the nearest-point table, the built target normals, the streams,
 * the device queues and the warm-ups -- and only the source stage of goicp_create is redone: the order of goicp_params::morton_sort
 * (computed on the device for modes 1 and 2), the gather with |p|, the centroid and the buffers sized by n_source (n_source may grow or
 * shrink).  Afterwards the handle answers every entry point bit for bit as a fresh handle created with the same params and target, the
 * new source, and the same per-handle options applied; only the wall-clock fields of goicp_poll may differ.
 *   persists: the params, goicp_set_icp_options / _gate / _robust, goicp_set_search_truncation, the progress callback (not called by the
 *             swap), goicp_set_shard, goicp_icp_shard_stats (accumulated since create);
 *   resets:   the goicp_icp_step pose, the goicp_poll snapshot (identity poses, best_sse 1e10, finished 0, counters 0), the neighbour cache,
 *             and the last run's goicp_icp_inliers / goicp_icp_robust_stats (refused until an ICP has run on the new cloud), so
 *             goicp_result_information is refused until a registration has finished on it.
 * GOICP_ERR_INVALID, the handle untouched: NULL arguments, n_source == 0, a non-finite coordinate, n_source above goicp_create's limit,
 * any call while a registration runs (between goicp_register_begin and goicp_register_end included).  After any other error (a HIP
 * failure in the middle of a swap) the handle is good for goicp_destroy only.  Sharded use: every rank swaps to the same cloud.
 */
int goicp_set_source(goicp_handle h, const float* source_xyz, size_t n_source);
/*
 * goicp_source_order_host (host only, no handle, no GPU): the source order of goicp_params::morton_sort = mode (0 input order, 1 30-bit
 * Morton curve over the cloud's bounding cube, 2 k-d order: recursive split of the longest bounding-box axis at the median rounded to
 * 256 / 64 / 16 / 4 points, down to single points; ties by index, -0 == +0).  perm[sorted position] = original index, n entries.
 * GOICP_ERR_INVALID: NULL arguments, n == 0 or above goicp_create's limit, a mode outside 0..2.
 */
int goicp_source_order_host(const float* xyz, size_t n, int32_t mode, int32_t* perm);
/*
 * Voxel-grid downsampling (PCL's VoxelGrid, Open3D's voxel_down_sample): one centroid per occupied cell of a grid of pitch `voxel`.
 * All three functions produce the same bits.  Float arithmetic is IEEE single precision, nothing fused:
 *   frame   mn_k = min_i x_ik, d_ik = x_ik - mn_k, E = max_ik d_ik;
 *   cell    c_ik = (int)floorf(d_ik / voxel); key = c_x | c_y << 21 | c_z << 42 (refused when E / voxel >= 2^21);
 *   sums    exact integers: the term of a coordinate is llrint(ldexp((double)d, s)), s = 62 - e - b with E < 2^e (frexp) and b the bit length
 *           of n (s = 0 when E == 0), so every per-cell sum S_k stays below 2^62 and the order of addition cannot matter;
 *   output  the m occupied cells in ascending key order; a cell of one point returns that point's own bits, any other cell
 *           (float)((double)mn_k + ldexp((double)S_k / (double)count, -s)).  Each centroid is within 2^-23 (E + max|x|) of the cell's fp64
 *           centroid.
 * out_xyz holds n x 3 floats (the first m x 3 are written), out_count (may be NULL) n ints (points per cell), *m the number of cells.
 * goicp_voxel_downsample_host runs on the host alone (no handle, no GPU).  goicp_voxel_downsample runs the reduction on the device: the
 * handle lends its device and stream, its state is untouched.
 * goicp_set_source_voxel reduces on the device and swaps: the raw cloud is uploaded once, only the reduced cloud and the permutation come
 * back.  Afterwards the handle answers every entry point bit for bit as after goicp_set_source(h, D, m) with D the output of
 * goicp_voxel_downsample_host -- D's order is the "original order" of goicp_transform_source and goicp_eval_correspondences -- and
 * everything goicp_set_source keeps and resets carries over.  *n_kept (may be NULL) = m.  Sharded use: every rank calls it with the same
 * cloud and voxel.
 * GOICP_ERR_INVALID, the handle untouched: NULL arguments, n == 0 or above goicp_create's limit, a non-finite coordinate, a voxel that is
 * <= 0, NaN or infinite, E / voxel >= 2^21, and for the two handle forms any call while a registration runs.
 */
int goicp_voxel_downsample_host(const float* xyz, size_t n, float voxel, float* out_xyz, int32_t* out_count, size_t* m);
int goicp_voxel_downsample(goicp_handle h, const float* xyz, size_t n, float voxel, float* out_xyz, int32_t* out_count, size_t* m);
int goicp_set_source_voxel(goicp_handle h, const float* xyz, size_t n, float voxel, size_t* n_kept);
/*
 * Radius outlier removal (PCL's RadiusOutlierRemoval, Open3D's remove_radius_outlier): a point is kept when at least min_neighbors other
 * points lie within `radius` of it.  The host function, the device function and the filtered swap produce the same bits.  Float
 * arithmetic is IEEE single precision, nothing fused:
 *   r2      = radius * radius;
 *   pair    for points i != j: dx = x_i - x_j, dy = y_i - y_j, dz = z_i - z_j, d2 = dx*dx + dy*dy + dz*dz evaluated left to right
 *           (symmetric in i and j); j is a neighbour of i iff j != i && d2 <= r2.  A duplicate of a point is its neighbour, a point is
 *           never its own;
 *   count   count_i = min(number of neighbours of i, min_neighbors): the count saturates, so every implementation may stop early;
 *   keep    point i is kept iff count_i == min_neighbors;
 *   output  the m kept points in input order with their own bits, their original indices (ascending), and count_i of all n points.
 * The definition names no grid: the implementations search a grid of pitch radius * 1.03125f built on the voxel operator's frame, which
 * only selects candidates (DESIGN 18 proves that it misses no pair).
 * out_xyz holds n x 3 floats (the first m x 3 are written), out_index (may be NULL) n ints (the first m are written), out_count (may be
 * NULL) n ints (all written), *m the number of points kept; m == 0 is a valid result.
 * goicp_radius_outlier_removal_host runs on the host alone (no handle, no GPU).  goicp_radius_outlier_removal runs on the device: the
 * handle lends its device and stream, its state is untouched.
 * GOICP_ERR_INVALID, nothing written: NULL arguments, n == 0 or above goicp_create's limit, a non-finite coordinate, a radius that is
 * <= 0, NaN or infinite or whose radius * radius is not a normal float, min_neighbors < 1, E / radius >= 2^16 (E the frame's largest
 * offset, as in the voxel operator), and for the handle form any call while a registration runs.
 */
int goicp_radius_outlier_removal_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, float* out_xyz, int32_t* out_index, int32_t* out_count, size_t* m);
int goicp_radius_outlier_removal(goicp_handle h, const float* xyz, size_t n, float radius, int32_t min_neighbors, float* out_xyz, int32_t* out_index, int32_t* out_count, size_t* m);
/*
 * The filtered swap: the voxel grid when voxel > 0, then the radius filter on the reduced cloud when radius > 0, then the swap.  The raw
 * cloud is uploaded once and the stages are chained on the device; only the final cloud and the permutation (and the 24 bytes of the
 * reduced cloud's bounding box) come back.  Afterwards the handle answers every entry point bit for bit as after goicp_set_source(h, D, m)
 * with D the composition of goicp_voxel_downsample_host and goicp_radius_outlier_removal_host -- D's order is the "original order" of
 * goicp_transform_source and goicp_eval_correspondences -- and everything goicp_set_source keeps and resets carries over.  With both
 * stages off it is goicp_set_source, with only `voxel` set goicp_set_source_voxel.  *n_kept (may be NULL) = m.
 * GOICP_ERR_INVALID, the handle untouched: a filter that keeps no point, radius > 0 with min_neighbors < 1, a negative or NaN voxel or
 * radius, everything the stages and goicp_set_source refuse, and any call while a registration runs.
 */
typedef struct goicp_source_filter { float voxel; float radius; int32_t min_neighbors; } goicp_source_filter;
void goicp_source_filter_default(goicp_source_filter* out);   /* all 0 = no stage */
int goicp_set_source_filtered(goicp_handle h, const float* xyz, size_t n, const goicp_source_filter* f, size_t* n_kept);
/*
 * Statistical outlier removal (PCL's StatisticalOutlierRemoval with setMeanK / setStddevMulThresh, Open3D's remove_statistical_outlier
 * with nb_neighbors / std_ratio): a point is dropped when its mean distance to its k = `neighbors` nearest neighbours lies more than
 * alpha = `std_ratio` standard deviations above the cloud's mean of that quantity.  The host function, the device function and the chained
 * swap produce the same bits.  Arithmetic is IEEE, nothing fused:
 *   pair    for points i != j, in float: dx = x_i - x_j, dy = y_i - y_j, dz = z_i - z_j, d2 = dx*dx + dy*dy + dz*dz evaluated left to right
 *           (the radius filter's expression, symmetric in i and j).  A duplicate of a point is its neighbour at distance 0, a point is
 *           never its own neighbour;
 *   nearest the n - 1 values d2(i, .) sorted ascending, the first k of them as a multiset (ties share a value: which tied point is taken
 *           cannot show).  s_i = sum of (double)sqrtf(d2) over them, added in ascending order, sqrtf correctly rounded;
 *           u_i = (float)(s_i / (double)k);
 *   image   U = max u_i.  U == 0: every point is kept and the threshold is 0.  Otherwise frexp(U) gives e with U < 2^e,
 *           q_i = (int64)floor(ldexp((double)u_i, 31 - e)), 0 <= q_i < 2^31, and the exact integer sums S1 = sum q_i,
 *           A = sum (q_i * q_i >> 32), B = sum (q_i * q_i & 0xffffffff): below 2^60 each, so the order of addition cannot matter;
 *   finish  in fp64, each operation rounded once: nd = (double)n, mean = (double)S1 / nd, S2 = ldexp((double)A, 32) + (double)B,
 *           var = (S2 - (double)S1 * mean) / (nd - 1), set to 0 unless var > 0, Tq = mean + (double)alpha * sqrt(var) -- PCL's
 *           (sum m^2 - (sum m)^2 / n) / (n - 1), Open3D's sample deviation;
 *   keep    point i is kept iff (double)q_i <= Tq.  The point with the smallest q always passes, so m >= 1.  The reported threshold is
 *           ldexp(Tq, e - 31); the quantisation step is below U * 2^-30;
 *   output  the m kept points in input order with their own bits, their original indices (ascending), u_i of all n points, the threshold.
 * The definition names no grid and nothing about the cloud's extent is refused: the implementations search grids of doubling pitch that
 * only select candidates.  A cloud whose d2 all underflow to 0 has u = 0 and keeps everything.
 * out_xyz holds n x 3 floats (the first m x 3 are written), out_index (may be NULL) n ints (the first m are written), out_mean_dist (may
 * be NULL) n floats (all written), *threshold (may be NULL) the threshold, *m the number of points kept.
 * goicp_statistical_outlier_removal_host runs on the host alone (no handle, no GPU).  goicp_statistical_outlier_removal runs on the
 * device: the handle lends its device and stream, its state is untouched.
 * GOICP_ERR_INVALID, nothing written: NULL arguments, n == 0 or above goicp_create's limit, a non-finite coordinate, neighbors outside
 * 1..GOICP_STAT_MAX_NEIGHBORS or above n - 1, a std_ratio that is negative, NaN or infinite, and for the handle form any call while a
 * registration runs.
 */
#define GOICP_STAT_MAX_NEIGHBORS 64
int goicp_statistical_outlier_removal_host(const float* xyz, size_t n, int32_t neighbors, float std_ratio, float* out_xyz, int32_t* out_index, float* out_mean_dist, double* threshold, size_t* m);
int goicp_statistical_outlier_removal(goicp_handle h, const float* xyz, size_t n, int32_t neighbors, float std_ratio, float* out_xyz, int32_t* out_index, float* out_mean_dist, double* threshold, size_t* m);
/*
 * The three-stage swap: the voxel grid when voxel > 0, then the statistical filter when stat_neighbors > 0, then the radius filter when
 * radius > 0, then the swap.  The raw cloud is uploaded once, every stage reads the previous stage's device buffer, and only the final
 * cloud and the permutation (and the 24 bytes of an intermediate cloud's bounding box) come back.  Afterwards the handle answers every
 * entry point bit for bit as after goicp_set_source(h, D, m) with D the composition of the host functions.  With the statistical stage
 * off it runs goicp_set_source_filtered.  *n_kept (may be NULL) = m.
 * GOICP_ERR_INVALID, the handle untouched: everything the stages and goicp_set_source_filtered refuse, a negative stat_neighbors,
 * stat_neighbors above the size of the cloud that reaches the stage minus one, a chain that keeps no point, and any call while a
 * registration runs.
 */
typedef struct goicp_source_pipeline { float voxel; int32_t stat_neighbors; float stat_std_ratio; float radius; int32_t min_neighbors; } goicp_source_pipeline;
void goicp_source_pipeline_default(goicp_source_pipeline* out);   /* all 0 = no stage */
int goicp_set_source_pipeline(goicp_handle h, const float* xyz, size_t n, const goicp_source_pipeline* p, size_t* n_kept);
/*
 * Exact self k-NN and normal estimation for any cloud (PCL's NormalEstimation with setKSearch and setViewPoint, Open3D's estimate_normals
 * with KDTreeSearchParamKNN plus orient_normals_towards_camera_location).  Each operator has a host function, a device function and a
 * numpy twin that produce the same bits.  Arithmetic is IEEE, nothing fused.
 *
 * Self k-NN: for every point i of the n points, its k nearest OTHER points.
 *   pair    the statistical filter's float expression: dx = x_i - x_j, dy = y_i - y_j, dz = z_i - z_j, d2 = dx*dx + dy*dy + dz*dz evaluated
 *           left to right.  A duplicate of a point is its neighbour at distance 0, a point is never its own neighbour;
 *   order   by the 64-bit key ((uint64)bits of d2 << 32) | j, ascending: d2 >= 0, so this is (d2, index) order, a total order -- ties at the
 *           k-th place go to the smaller index (goicp_knn_query's rule; unlike the statistical filter's multiset, which tied point is
 *           taken shows here);
 *   output  out_index: n x k int32, row i = the k smallest keys' indices, ascending by key; out_dist_sq (may be NULL): n x k floats, their d2.
 * The definition names no grid and nothing about the cloud's extent is refused: the implementations search grids of doubling pitch that
 * only select candidates.
 * GOICP_ERR_INVALID, nothing written: NULL arguments, n == 0 or above goicp_create's limit, a non-finite coordinate, k outside
 * 1..GOICP_KNN_SELF_MAX or above n - 1, and for the handle form any call while a registration runs.
 *
 * Normals: k in 3..GOICP_KNN_SELF_MAX counts the point itself (as goicp_icp_options.normal_k does), k - 1 <= n - 1; vp (may be NULL) is a
 * viewpoint.  The neighbourhood of i is i itself followed by its k - 1 nearest others in key order (the self k-NN at k - 1).  Everything
 * below is fp64, each operation rounded once, and uses only + - * / sqrt (and negation, comparisons, |.|):
 *   offsets e_j = (double)x_j - (double)x_i per component; e_0 = (0, 0, 0) is the point's own.  Offsets from the point keep every error
 *           relative to the neighbourhood's size, not to |x|;
 *   mean    m = (sum of e_j) / (double)k, the sum added sequentially in neighbourhood order from 0;
 *   cov     d_j = e_j - m; the six entries C_ab = sum over j of d_ja * d_jb, each product rounded, added sequentially in the same order
 *           from 0;
 *   eigen   cyclic Jacobi on the full 3 x 3 matrix A = C with V = I, the pairs (p, q) = (0,1), (0,2), (1,2) per sweep.  A pair is skipped
 *           when apq == 0 or apq*apq <= 1e-24 * |app*aqq| (apq = A[p][q]).  Otherwise da = aqq - app, db = apq + apq,
 *           tn = (da >= 0 ? db : -db) / (|da| + sqrt(da*da + db*db)), cs = 1 / sqrt(1 + tn*tn), sn = cs * tn, and for r = 0, 1, 2 in turn:
 *           columns (A[r][p], A[r][q]) <- (cs*A[r][p] - sn*A[r][q], sn*A[r][p] + cs*A[r][q]), then rows
 *           (A[p][r], A[q][r]) <- (cs*A[p][r] - sn*A[q][r], sn*A[p][r] + cs*A[q][r]), then the columns of V as those of A.  The
 *           iteration stops after a sweep that skipped all three pairs, or after 32 sweeps;
 *   normal  l_c = A[c][c].  The column of V with the smallest l_c, the lowest c on equal values: v.  len = sqrt((v0*v0 + v1*v1) + v2*v2),
 *           n_c = (float)(v_c / len);
 *   flat    with a <= b <= c the three l sorted: c <= 0 (every neighbour coincides with the point) gives normal (0, 0, 0), variation 0;
 *   variation  (float)((a > 0 ? a : 0) / ((a + b) + c)): PCL's curvature, in [0, 1/3];
 *   sign    on the float normal.  With a viewpoint, d = ((double)n_0 * ((double)vp_0 - (double)x_i0) + (double)n_1 * (...)) + (double)n_2 * (...);
 *           d < 0 negates the normal.  With no viewpoint or d == 0, the normal is negated when its first non-zero component is negative.
 *           A zero component is written as +0;
 *   output  out_normals: n x 3 floats in input order; out_variation (may be NULL): n floats; out_index (may be NULL): n x (k - 1) int32,
 *           the neighbours used.
 * GOICP_ERR_INVALID, nothing written: what the self k-NN refuses of the cloud, k outside 3..GOICP_KNN_SELF_MAX, k - 1 > n - 1, a
 * non-finite viewpoint, and for the handle form any call while a registration runs.
 * The _host forms run on the host alone (no handle, no GPU).  The handle forms run on the device: the handle lends its device and stream,
 * its state is untouched.
 */
#define GOICP_KNN_SELF_MAX 32
int goicp_knn_self_host(const float* xyz, size_t n, int32_t k, int32_t* out_index, float* out_dist_sq);
int goicp_knn_self(goicp_handle h, const float* xyz, size_t n, int32_t k, int32_t* out_index, float* out_dist_sq);
int goicp_estimate_normals_host(const float* xyz, size_t n, int32_t k, const float vp[3], float* out_normals, float* out_variation, int32_t* out_index);
int goicp_estimate_normals(goicp_handle h, const float* xyz, size_t n, int32_t k, const float vp[3], float* out_normals, float* out_variation, int32_t* out_index);
/*
 * FPFH descriptors and descriptor matching (Rusu, Blodow and Beetz 2009: the Fast Point Feature Histogram, 33 bins; PCL's FPFHEstimation
 * with setKSearch, Open3D's compute_fpfh_feature with KDTreeSearchParamKNN, and the nearest-descriptor search both libraries' feature
 * matching starts from).  Each operator has a host function, a device function and a numpy twin that produce the same bits.  Arithmetic
 * is IEEE, nothing fused.
 *
 * FPFH: n points, n float normals (the caller's own, or goicp_estimate_normals' output), k in 1..GOICP_KNN_SELF_MAX, k <= n - 1, counts
 * the nearest OTHER points.  The neighbourhood of i is row i of the self k-NN at k: key order, with that operator's float d2.  Everything
 * below is fp64 (every float widened first), each operation rounded once, and uses only + - * / sqrt, comparisons, |.| and floor:
 *   pair    (i, j): d = p_j - p_i per component, l2 = (d0*d0 + d1*d1) + d2*d2.  The pair is SKIPPED when !(l2 > 0) or when either normal is
 *           all zeros.  l = sqrt(l2), a1 = (n_i . d) / l, a2 = (n_j . d) / l; every dot is (x*x' + y*y') + z*z'.
 *           If |a1| < |a2| the frame's source is j: ns = n_j, nt = n_i, d = -d, f3 = -a2.  Otherwise ns = n_i, nt = n_j, f3 = a1 (PCL's
 *           computePairFeatures).  v = d x ns, every component x*y - z*w with both products rounded; vl2 formed as l2 was; the pair is
 *           skipped when !(vl2 > 0).  v_c = v_c / sqrt(vl2), w = ns x v, f2 = v . nt, x = ns . nt, y = w . nt;
 *   bins    b3 = clamp(floor(11.0 * ((f3 + 1.0) * 0.5)), 0, 10), clamped before the conversion to an integer; b2 the same over f2.
 *           b1 is the bin of atan2(y, x) among 11 equal bins of [-pi, pi), decided without atan2: with (a, b) = (-x, -y), whose angle is
 *           atan2(y, x) + pi in [0, 2 pi), and (C_k, S_k) = GOICP_FPFH_COS[k - 1], GOICP_FPFH_SIN[k - 1], the doubles nearest the cosine
 *           and sine of 2 pi k / 11, cross_k = C_k*b - S_k*a with both products rounded; the test of k holds when b < 0 || cross_k >= 0
 *           for k <= 5 and when b < 0 && cross_k >= 0 for k >= 6; b1 = the number of k in 1..10 whose test holds.  x == 0 && y == 0
 *           gives bin 5 (atan2(0, 0) = 0);
 *   SPFH    exact integer counts c_i[33] over the k neighbours of i in PCL's layout: c[b1], c[11 + b2], c[22 + b3] each go up by one per
 *           pair; skipped pairs count nowhere;
 *   FPFH    inc = 100.0 / (double)k.  For every bin, a_b = sum over the row of (((double)c_jb * inc) * w_j), added in key order from 0,
 *           w_j = 1.0 / (double)d2_j (the squared-distance weight of PCL and Open3D); neighbours with d2_j == 0 are skipped.  For each of
 *           the three groups of 11 bins, s_g = sum of a_b ascending in b from 0; when s_g > 0, a_b = a_b * (100.0 / s_g).
 *           out_b = (float)(a_b + (double)c_ib * inc);
 *   output  out_fpfh: n x GOICP_FPFH_DIM floats in input order; out_spfh_counts (may be NULL): n x GOICP_FPFH_DIM uint8, the counts c_i.
 * GOICP_ERR_INVALID, nothing written: what goicp_knn_self refuses, a NULL or non-finite normal, and for the handle form any call while a
 * registration runs.
 *
 * Matching: for every one of n_q query descriptors (GOICP_FPFH_DIM floats each) the nearest of n_t target descriptors.  Float:
 *   pair    d2(q, t) = sum over b = 0..32 of (q_b - t_b) * (q_b - t_b), added left to right from 0;
 *   order   by the key ((uint64)bits of d2 << 32) | t, ascending: ties go to the smaller index;
 *   output  out_index (n_q int32), out_d2 (n_q floats): the smallest key; out_d2_second (n_q floats): the d2 of the second-smallest key,
 *           +inf when n_t == 1 (for the caller's ratio test); out_mutual (may be NULL; n_q uint8): 1 iff the query is in turn the
 *           smallest-key match of its target, the same rule with the two sets exchanged, else 0.
 * The cost is n_q * n_t * 33 subtractions, products and additions in the order above (no matrix instruction can keep that order): it
 * is meant for downsampled clouds of some 10^4 descriptors, not for raw scans.
 * GOICP_ERR_INVALID, nothing written: NULL arguments (out_mutual aside), n_q == 0, n_t == 0, a size above goicp_create's limit, a
 * non-finite descriptor, and for the handle form any call while a registration runs.
 * goicp_match_features_tile(): the number of target descriptors the device kernel stages per tile (tests cut their sizes around it).
 */
#define GOICP_FPFH_DIM 33
#define GOICP_FPFH_COS { 0x1.aeb8c8764f0bap-1, 0x1.a9628d9c712b6p-2, -0x1.2375f640f44dbp-3, -0x1.4f49e7f775887p-1, -0x1.eb42a9bcd5057p-1, \
                         -0x1.eb42a9bcd5057p-1, -0x1.4f49e7f775887p-1, -0x1.2375f640f44dbp-3, 0x1.a9628d9c712b6p-2, 0x1.aeb8c8764f0bap-1 }
#define GOICP_FPFH_SIN { 0x1.14cedf8bb580bp-1, 0x1.d1bb48eee2c13p-1, 0x1.fac9e043842efp-1, 0x1.82f19bb3a28a1p-1, 0x1.207e7fd768dbfp-2, \
                         -0x1.207e7fd768dbfp-2, -0x1.82f19bb3a28a1p-1, -0x1.fac9e043842efp-1, -0x1.d1bb48eee2c13p-1, -0x1.14cedf8bb580bp-1 }
int goicp_fpfh_host(const float* xyz, const float* normals, size_t n, int32_t k, float* out_fpfh, uint8_t* out_spfh_counts);
int goicp_fpfh(goicp_handle h, const float* xyz, const float* normals, size_t n, int32_t k, float* out_fpfh, uint8_t* out_spfh_counts);
int goicp_match_features_host(const float* query, size_t n_q, const float* target, size_t n_t, int32_t* out_index, float* out_d2, float* out_d2_second,
                              uint8_t* out_mutual);
int goicp_match_features(goicp_handle h, const float* query, size_t n_q, const float* target, size_t n_t, int32_t* out_index, float* out_d2,
                         float* out_d2_second, uint8_t* out_mutual);
int goicp_match_features_tile(void);
/*
 * Euclidean / DBSCAN clustering (PCL's EuclideanClusterExtraction, Open3D's cluster_dbscan): connected components under a distance, and
 * the filter "keep the largest clusters" built on it.  The host functions, the device functions and the clustered swap produce the same
 * bits.  The only float expression is the radius filter's pair; everything else is integers:
 *   r2      = radius * radius;
 *   pair    for points i != j: dx = x_i - x_j, dy = y_i - y_j, dz = z_i - z_j, d2 = dx*dx + dy*dy + dz*dz evaluated left to right; j is a
 *           neighbour of i iff j != i && d2 <= r2.  A duplicate of a point is its neighbour, a point is never its own;
 *   core    point i is core iff min(number of neighbours of i, min_neighbors) == min_neighbors (the radius filter's saturating count).
 *           min_neighbors == 0 makes every point core: PCL's Euclidean clustering.  min_neighbors >= 1 is DBSCAN with
 *           min_points = min_neighbors + 1;
 *   cluster a connected component of the core points under the neighbour relation;
 *   border  a point that is not core but has a core neighbour joins the cluster of the core neighbour j with the smallest 64-bit key
 *           ((uint64)bits of d2 << 32) | j.  A border point never connects two clusters;
 *   noise   every other point: label -1;
 *   labels  the c clusters are numbered 0..c-1 in ascending order of their smallest core member's index; sizes[l] counts the core and the
 *           border members of cluster l;
 *   select  (the filter) the clusters ranked by size descending, ties to the smaller label; of those with size >= max(min_size, 1) the
 *           first max_clusters are kept (max_clusters == 0: all of them).  The output is the m points of the kept clusters in input
 *           order with their own bits, their original indices (ascending) and their labels.
 * The definition names no grid: the implementations search the radius filter's grid.
 * goicp_cluster: out_label holds n ints (all written), out_sizes (may be NULL) n ints (the first c are written), *n_clusters = c; c == 0
 * (all noise) is a valid result.  goicp_cluster_filter: out_xyz holds n x 3 floats (the first m x 3 are written), out_index and out_label
 * (each may be NULL) n ints (the first m are written), *m the number of points kept; m == 0 is a valid result.
 * The _host forms run on the host alone (no handle, no GPU).  The handle forms run on the device: the handle lends its device and stream,
 * its state is untouched.
 * goicp_set_source_clustered chains the stages of goicp_set_source_pipeline (p; NULL = none of them), then the cluster selection when
 * s->radius > 0, then the swap, on the device behind one upload.  Afterwards the handle answers every entry point bit for bit as after
 * goicp_set_source(h, D, m) with D the composition of the host functions.  With s->radius == 0 it is goicp_set_source_pipeline.
 * *n_kept (may be NULL) = m.
 * GOICP_ERR_INVALID, nothing written or the handle untouched: what goicp_radius_outlier_removal refuses except min_neighbors == 0, a
 * negative min_neighbors, min_size or max_clusters, for the swap everything goicp_set_source_pipeline refuses, a negative or NaN
 * s->radius and a selection that keeps no point, and for the handle forms any call while a registration runs.
 */
int goicp_cluster_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t* out_label, int32_t* out_sizes, size_t* n_clusters);
int goicp_cluster(goicp_handle h, const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t* out_label, int32_t* out_sizes, size_t* n_clusters);
typedef struct goicp_cluster_select { float radius; int32_t min_neighbors; int32_t min_size; int32_t max_clusters; } goicp_cluster_select;
void goicp_cluster_select_default(goicp_cluster_select* out);   /* all 0 = no stage */
int goicp_cluster_filter_host(const float* xyz, size_t n, const goicp_cluster_select* s, float* out_xyz, int32_t* out_index, int32_t* out_label, size_t* m);
int goicp_cluster_filter(goicp_handle h, const float* xyz, size_t n, const goicp_cluster_select* s, float* out_xyz, int32_t* out_index, int32_t* out_label, size_t* m);
int goicp_set_source_clustered(goicp_handle h, const float* xyz, size_t n, const goicp_source_pipeline* p, const goicp_cluster_select* s, size_t* n_kept);
/*
 * RANSAC plane segmentation (PCL's SACSegmentation with SACMODEL_PLANE / SAC_RANSAC plus ExtractIndices(negative), Open3D's segment_plane
 * plus select_by_index(invert=True)): the dominant planes of a cloud -- the floor, table or wall an object stands on -- and the filter
 * "drop their points" built on it.  The host functions, the device functions and the segmented swap produce the same bits.  Arithmetic is
 * IEEE, nothing fused.  With T = iterations (0 means 1000) and P = max_planes (0 means 1):
 *   rounds  round p = 0, 1, ... < P works on the points no earlier round labelled, in input order: n_p of them.  A round with n_p < 3 finds
 *           nothing and ends the search, and so does a round whose best count is below max(min_inliers, 3);
 *   draw    hypothesis t < T of round p takes three distinct positions a, b, c of the remaining cloud from a counter-based generator:
 *           h(c) = the splitmix64 finaliser of z = seed + (c + 1) * 0x9E3779B97F4A7C15 (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 *           z *= 0x94D049BB133111EB, z ^= z >> 31; all mod 2^64) at the counters 3 (p T + t) + {0, 1, 2}: a = h_0 mod n_p; b = h_1 mod
 *           (n_p - 1), incremented when >= a; c = h_2 mod (n_p - 2), incremented when >= min(a, b), then again when >= max(a, b).  Integers
 *           only, no state: any hypothesis can be computed alone;
 *   plane   in fp64, each operation rounded once: u = p_b - p_a, v = p_c - p_a on the widened floats, n = u x v (each component x*y - z*w
 *           with both products rounded), l2 = (n_0 n_0 + n_1 n_1) + n_2 n_2.  The hypothesis is degenerate when !(l2 > 0) or a component of
 *           the float normal n_c = (float)(n_c / sqrt(l2)) is not finite: it scores 0 and can never be the best.  The sign is the normals
 *           operator's on the float normal (the first non-zero component positive, a zero written as +0); the anchor is point a's own bits;
 *   pair    in float, left to right: e = ((x_0 - a_0) * n_0 + (x_1 - a_1) * n_1) + (x_2 - a_2) * n_2; the point is an inlier iff
 *           fabsf(e) <= distance (a NaN compares false).  Offsets from the anchor keep the error relative to the cloud's extent, not to |x|;
 *   score   the exact integer count over all n_p points; the best is the largest count, ties to the smallest t;
 *   refit   (refine = 1) one least-squares refit over the best hypothesis' inliers, with exact integer moments.  The frame is the voxel
 *           operator's over the round's cloud: mn_k, d = x - mn_k in float, E = max d, E < 2^e by frexp;
 *           q_k = llrint(ldexp((double)d_k, 31 - e)) in [0, 2^31); the sums m (the count), S_a = sum q_a and P_ab = sum q_a q_b for the
 *           six pairs a <= b, the P_ab as sum (prod >> 32) and sum (prod & 0xffffffff): 16 words, each below 2^60, so the order of addition
 *           cannot matter.  From those words, on the host in both paths: C_ab = ldexp((double)(m P_ab - S_a S_b), -2 (31 - e)) /
 *           ((double)m * (double)m), the integer formed exactly in 128 bits and converted to double correctly rounded; the normals
 *           operator's Jacobi on C; the column of the smallest eigenvalue (the lowest index on equal values) normalised, cast and signed as
 *           above; the anchor (float)((double)mn_k + ldexp((double)S_k / (double)m, -(31 - e))), the voxel operator's centroid.  The pair
 *           re-selects against the refit plane, which is adopted iff its count is >= the hypothesis' count (a refit without a finite
 *           non-zero normal is not adopted); `refined` reports which stands;
 *   output  per point a label: -1, or the index of the plane that took it; per plane a goicp_plane with `inliers` the count of the plane
 *           that stands, `hypothesis` the best t, and d = (float)(-((n_0 p_0 + n_1 p_1) + n_2 p_2)) in fp64 on the widened floats: the
 *           ax + by + cz + d = 0 form PCL and Open3D return.  The filter returns the points labelled -1 in input order with their own bits
 *           and their original indices (ascending).
 * goicp_segment_plane: out_label holds n ints (all written), out_planes room for max_planes records (GOICP_PLANE_MAX_PLANES always
 * suffices; the first *n_planes are written).  goicp_plane_filter: out_xyz holds n x 3 floats (the first m x 3 are written), out_index (may
 * be NULL) n ints (the first m), out_planes and n_planes (each may be NULL) as above.  Zero planes, m == n and m == 0 are valid results.
 * The _host forms run on the host alone (no handle, no GPU).  The handle forms run on the device: the handle lends its device and stream,
 * its state is untouched; only the best key and plane of a round, the refit's 16 words and the final cloud come back.
 * goicp_set_source_segmented is the full chain behind one upload: voxel -> statistical -> radius (p; NULL = none of them) -> plane removal
 * (pl; NULL or pl->distance == 0 = no stage) -> cluster selection (s; NULL or s->radius == 0 = no stage) -> swap.  Afterwards the handle
 * answers every entry point bit for bit as after goicp_set_source(h, D, m) with D the composition of the host functions.  With the plane
 * stage off it is goicp_set_source_clustered.  *n_kept (may be NULL) = m.
 * GOICP_ERR_INVALID, nothing written or the handle untouched: NULL arguments, n == 0 or above goicp_create's limit, a non-finite
 * coordinate, a distance that is <= 0, NaN or infinite (for the swap: negative or NaN; 0 is "no stage"), iterations outside
 * 0..GOICP_PLANE_MAX_ITERATIONS, max_planes outside 0..GOICP_PLANE_MAX_PLANES, a negative min_inliers (a min_inliers above n is legal and
 * finds no plane), refine outside 0..1, for the swap everything goicp_set_source_clustered refuses and a chain that keeps no point, and
 * for the handle forms any call while a registration runs.
 */
#define GOICP_PLANE_MAX_ITERATIONS 65536
#define GOICP_PLANE_MAX_PLANES 8
typedef struct goicp_plane_select {
    float    distance;      /* inlier threshold; 0 = no stage (the swap) */
    int32_t  iterations;    /* hypotheses per round; 0 = 1000 */
    int32_t  refine;        /* 1 = least-squares refit over the best hypothesis' inliers */
    int32_t  max_planes;    /* rounds at most; 0 = 1 */
    int32_t  min_inliers;   /* a best count below max(min_inliers, 3) ends the search */
    uint64_t seed;
} goicp_plane_select;
typedef struct goicp_plane {
    float   normal[3];
    float   point[3];       /* the anchor: a point of the plane */
    float   d;              /* normal . x + d = 0 */
    int32_t inliers;
    int32_t hypothesis;     /* the best t of the round */
    int32_t refined;        /* 1: the refit stands */
} goicp_plane;
void goicp_plane_select_default(goicp_plane_select* out);   /* all 0 = no stage */
int goicp_segment_plane_host(const float* xyz, size_t n, const goicp_plane_select* sel, int32_t* out_label, goicp_plane* out_planes, size_t* n_planes);
int goicp_segment_plane(goicp_handle h, const float* xyz, size_t n, const goicp_plane_select* sel, int32_t* out_label, goicp_plane* out_planes, size_t* n_planes);
int goicp_plane_filter_host(const float* xyz, size_t n, const goicp_plane_select* sel, float* out_xyz, int32_t* out_index, goicp_plane* out_planes,
                            size_t* n_planes, size_t* m);
int goicp_plane_filter(goicp_handle h, const float* xyz, size_t n, const goicp_plane_select* sel, float* out_xyz, int32_t* out_index, goicp_plane* out_planes,
                       size_t* n_planes, size_t* m);
int goicp_set_source_segmented(goicp_handle h, const float* xyz, size_t n, const goicp_source_pipeline* p, const goicp_plane_select* pl,
                               const goicp_cluster_select* s, size_t* n_kept);
/*
 * RANSAC pose estimation from correspondences (PCL's SampleConsensusPrerejective, Open3D's registration_ransac_based_on_correspondence):
 * the rigid poses that the most of M putative correspondences (source index, target index) agree with -- the step from
 * goicp_match_features to start poses for goicp_icp_run_batch.  The host function and the device function produce the same bits, and two
 * device runs the same bytes.  Arithmetic is IEEE, nothing fused; fp64 operations are rounded once each and are + - * / sqrt and
 * comparisons only.  With T = iterations (0 means 100000), K = max_poses (0 means 1), s_j / m_j the source / target point of
 * correspondence j, and dot3(a, b) = (a_0 b_0 + a_1 b_1) + a_2 b_2:
 *   draw    hypothesis t < T takes three distinct correspondences a, b, c: the plane operator's draw at the counters 3 t + {0, 1, 2}
 *           (its round p = 0) over M positions;
 *   reject  (edge_similarity = sigma > 0) in fp64 on the widened floats, for each of the edges (a, b), (b, c), (c, a): d = p_second -
 *           p_first, ls2 = dot3(d, d) on the source points and lt2 on the target points; the hypothesis is rejected unless every edge has
 *           min(ls2, lt2) >= (sigma sigma) max(ls2, lt2), the product sigma sigma formed once in fp64 from the widened float.  Open3D's
 *           CorrespondenceCheckerBasedOnEdgeLength and PCL's polygon pre-rejector, without the square roots.  A rejected hypothesis scores 0;
 *   pose    in fp64 from a cross-covariance H (target rows, source columns) and the centroids cs, ct -- one text for the hypothesis and
 *           the refit.  For a triple: cs_k = ((sa_k + sb_k) + sc_k) / 3.0, ct likewise, H_ab = ((ma_a - ct_a)(sa_b - cs_b) +
 *           (mb_a - ct_a)(sb_b - cs_b)) + (mc_a - ct_a)(sc_b - cs_b).  Then K = H^T H, K_ab = dot3(column a of H, column b of H); the
 *           normals operator's cyclic Jacobi on K (rotations (0,1), (0,2), (1,2), at most 32 sweeps, the same skip and stop tests) gives
 *           l_c = the diagonal and the columns of V; they are put in descending order of l by the exchanges (0,1), (1,2), (0,1), each made
 *           only when the later l is strictly larger (equal values keep the lower index first).  Degenerate when !(l_1 > 0): collinear
 *           or coincident points.  u_k = H v_k (u_ka = dot3(row a of H, v_k)), u_k /= sqrt(dot3(u_k, u_k)) for k = 0, 1;
 *           u_1 -= dot3(u_0, u_1) u_0 and u_1 /= sqrt(dot3(u_1, u_1)) again; u_2 = u_0 x u_1 and v_2 = v_0 x v_1 (each component
 *           x*y - z*w with both products rounded); R_ab = (float)((u0_a v0_b + u1_a v1_b) + u2_a v2_b), a proper rotation by
 *           construction; t_a = (float)(ct_a - dot3(widened float row a of R, cs)).  A pose with a non-finite entry is degenerate.  A
 *           degenerate hypothesis scores 0 and can never be returned;
 *   pair    in float, left to right: y_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a, e_a = y_a - m_a, d2 = (e_0 e_0 + e_1 e_1) + e_2 e_2;
 *           correspondence j is an inlier iff d2 <= distance * distance, the product formed once in float (a NaN compares false);
 *   score   the exact integer count over all M correspondences; key = (count << 32) | ~t as 64 unsigned bits;
 *   poses   the K largest keys (the largest count first, ties to the smallest t) whose count is at least max(min_inliers, 3), in
 *           descending key order.  *n_poses may be 0, a valid result;
 *   refit   (refine = 1, for each returned pose on its own) one least-squares refit over the pose's inliers, with exact integer moments.
 *           Each side has the voxel operator's frame over the M points that the correspondences name on it (a point named twice counts
 *           once for the frame): mn_k, d = x - mn_k in float, E = max d, E < 2^e by frexp; q_k = llrint(ldexp((double)d_k, 31 - e)) in
 *           [0, 2^31).  The sums over the inliers: m (the count), Ss_b = sum qs_b, St_a = sum qt_a and P_ab = sum qt_a qs_b for the nine
 *           pairs, the P_ab as sum (prod >> 32) and sum (prod & 0xffffffff): 25 words, each below 2^60, so the order of addition cannot
 *           matter.  From those words, on the host in both paths: H_ab = ldexp((double)(m P_ab - St_a Ss_b), -(31 - e_s) - (31 - e_t)) /
 *           ((double)m * (double)m), the integer formed exactly in 128 bits and converted to double correctly rounded; cs_k =
 *           (double)mn_k + ldexp((double)Ss_k / (double)m, -(31 - e_s)), the voxel operator's centroid kept in fp64, ct likewise; then
 *           `pose` above.  The pair re-selects against the refit pose, which is adopted iff it is not degenerate and its count is >= the
 *           hypothesis' count; `refined` reports which stands;
 *   output  out_poses[i]: R (row-major) and t of the pose that stands, `inliers` its count, `hypothesis` its t, `refined`;
 *           out_inlier[j] (may be NULL; M bytes): the pair's verdict on correspondence j under out_poses[0], all 0 when there is no pose.
 * out_poses has room for max_poses records (GOICP_RANSAC_POSE_MAX_POSES always suffices; the first *n_poses are written).  A source or
 * target index may occur in several correspondences.  The _host form runs on the host alone (no handle, no GPU).  The handle form runs on
 * the device: the handle lends its device and stream, its state is untouched; 56 bytes per returned pose, the refit's 200 per pose and the
 * M verdicts come back.
 * goicp_select_matches (host only, linear in n_q) turns goicp_match_features' output into correspondences: query q is kept iff
 * (!require_mutual || mutual[q]) and, with ratio != 0, d2[q] <= (ratio * ratio) * d2_second[q] in float with ratio * ratio formed once
 * (Lowe's ratio test on squared distances; a d2_second of +inf passes).  out_corr holds n_q x 2 ints; the *M kept pairs (q, index[q]) are
 * written in ascending q.  mutual may be NULL when require_mutual == 0.
 * goicp_ransac_pose_tile() / goicp_ransac_pose_block(): the hypotheses the device score kernel stages per LDS tile and the correspondences
 * of one of its workgroups (tests cut their sizes around them).
 * GOICP_ERR_INVALID, nothing written and the handle untouched: NULL arguments, M < 3, M, n_s or n_t above goicp_create's limit or a cloud
 * of no points, an index of corr out of range, a non-finite coordinate, a distance that is <= 0, NaN or infinite, iterations outside
 * 0..GOICP_RANSAC_POSE_MAX_ITERATIONS, max_poses outside 0..GOICP_RANSAC_POSE_MAX_POSES, refine outside 0..1, an edge_similarity outside
 * [0, 1] or NaN, a negative min_inliers (one above M is legal and finds no pose), for the handle form any call while a registration runs;
 * for goicp_select_matches NULL arguments (mutual only with require_mutual != 0), n_q == 0 or above the limit, a negative, NaN or infinite
 * ratio, require_mutual outside 0..1.
 */
#define GOICP_RANSAC_POSE_MAX_ITERATIONS (1 << 20)
#define GOICP_RANSAC_POSE_MAX_POSES 64
typedef struct goicp_ransac_pose_select {
    float    distance;         /* inlier threshold on |R s + t - m|; > 0, finite */
    int32_t  iterations;       /* hypotheses; 0 = 100000 */
    int32_t  refine;           /* 1 = least-squares refit over each returned pose's inliers */
    int32_t  max_poses;        /* poses returned at most; 0 = 1 */
    int32_t  min_inliers;      /* poses with a count below max(min_inliers, 3) are not returned */
    float    edge_similarity;  /* 0 = no pre-rejection; else in (0, 1] (Open3D's default is 0.9) */
    uint64_t seed;
} goicp_ransac_pose_select;
typedef struct goicp_ransac_pose_result {
    float   R[9];              /* row-major: y = R x + t takes the source onto the target */
    float   t[3];
    int32_t inliers;
    int32_t hypothesis;        /* the t of the hypothesis */
    int32_t refined;           /* 1: the refit stands */
} goicp_ransac_pose_result;
void goicp_ransac_pose_select_default(goicp_ransac_pose_select* out);   /* refine 1, edge_similarity 0.9, the rest 0 (distance is to be set) */
int goicp_ransac_pose_host(const float* src, size_t n_s, const float* tgt, size_t n_t, const int32_t* corr, size_t M, const goicp_ransac_pose_select* sel,
                           goicp_ransac_pose_result* out_poses, size_t* n_poses, uint8_t* out_inlier);
int goicp_ransac_pose(goicp_handle h, const float* src, size_t n_s, const float* tgt, size_t n_t, const int32_t* corr, size_t M,
                      const goicp_ransac_pose_select* sel, goicp_ransac_pose_result* out_poses, size_t* n_poses, uint8_t* out_inlier);
int goicp_select_matches(const int32_t* index, const float* d2, const float* d2_second, const uint8_t* mutual, size_t n_q, float ratio, int32_t require_mutual,
                         int32_t* out_corr, size_t* M);
int goicp_ransac_pose_tile(void);
int goicp_ransac_pose_block(void);
/* SSEThresh = mse_threshold * inlierNum and inlierNum = (int)(N * (1 - trim_fraction))
 * (src/goicp/jly_goicp.cpp:198-208; FastGoICP::sse_threshold, src/fgoicp/fgoicp.hpp:23) as the engine uses them */
int goicp_thresholds(goicp_handle h, float* sse_threshold, int32_t* inliers);
/* HIP device ordinal the engine lives on.  Every entry point makes it current for the calling thread
 * (HIP's current device is per thread) and restores the caller's afterwards. */
int goicp_device(goicp_handle h, int32_t* ordinal);

/* DT3D geometry (src/goicp/jly_3ddt.h:100-111) and the grid itself ([z][y][x], V^3 floats) */
int goicp_dt_info(goicp_handle h, int32_t* V, double* scale, double origin_xyz[3]);
int goicp_dt_download(goicp_handle h, float* grid);

/* ---- bounds operator ------------------------------------------------------------------------
 * Registration::compute_sse_error(RotNode&, std::vector<TransNode>&, bool fix_rot, StreamPool&)
 * (src/fgoicp/registration.hpp:97, registration.cu:88-151) == the inner body of GoICP::InnerBnB
 * (src/goicp/jly_goicp.cpp:262-315).  cubes: B x {centre x,y,z, child width w}.
 * level < 0  <=> fix_rot (no rotation uncertainty radius); otherwise the radii of rotation level
 * `level` (maxRotDis[level], src/goicp/jly_goicp.cpp:148-160) are subtracted. */
int goicp_eval_bounds(goicp_handle h, const float R[9], const float* cubes, size_t B, int32_t level,
                      float* ub, float* lb);

/* batched form: K rotations, B cube records (24 bytes each), each naming its rotation */
typedef struct goicp_cube {
	float tx, ty, tz;  /* cube centre */
	float delta;       /* translation uncertainty radius sqrt(3)/2*w (src/goicp/jly_goicp.cpp:263) */
	float coeff;       /* rotation uncertainty coefficient (goicp_rot_coeff(level)), 0 for fix_rot */
	int32_t rot;       /* index into rots */
} goicp_cube;
int goicp_eval_bounds_batch(goicp_handle h, const float* rots /* K x 9 */, size_t K,
                            const goicp_cube* cubes, size_t B, float* ub, float* lb);
/* device-resident form (no host copies): all four pointers are device pointers; stream = a
 * hipStream_t (NULL = the engine's own stream); asynchronous. */
int goicp_eval_bounds_device(goicp_handle h, const void* d_rots, const void* d_cubes, size_t B,
                             void* d_ub, void* d_lb, void* stream);
/* the same for a batch of UNRELATED cubes (arbitrary rotations and translations in any order -- what the four-argument
 * Registration::compute_sse_error may be handed, and SURVEY's microbench): the cubes are first bucketed on the device by (rotation,
 * pass, translation cell) with a counting sort, evaluated in that order and written back in the caller's order.  Bounds are per
 * cube, so not a bit changes; 65 536 unrelated cubes on the bunny take 2.3 ms instead of 3.75.  n_rots = entries of the rotation
 * table (1..16).  The search itself never needs this: its expansions arrive grouped by search, eight siblings at a time. */
int goicp_eval_bounds_device_grouped(goicp_handle h, const void* d_rots, size_t n_rots, const void* d_cubes, size_t B,
                                     void* d_ub, void* d_lb, void* stream);
int goicp_time_bounds_device_grouped(goicp_handle h, const void* d_rots, size_t n_rots, const void* d_cubes, size_t B,
                                     void* d_ub, void* d_lb, int32_t iters, float* ms_per_call);
/* min of n device floats and (d_argmin != NULL) the first index attaining it -- what a search does with a batch's upper
 * bounds (incumbent = smallest ub, first child on ties: jly_goicp.cpp:319-324); one workgroup, asynchronous on `stream`
 * (NULL = the engine's own).  d_values must be 16-byte aligned. */
int goicp_reduce_min_device(goicp_handle h, const void* d_values, size_t n, void* d_min, void* d_argmin, void* stream);
/* average duration (ms, HIP events on the launch stream) of `iters` back-to-back launches */
int goicp_time_bounds_device(goicp_handle h, const void* d_rots, const void* d_cubes, size_t B,
                             void* d_ub, void* d_lb, int32_t iters, float* ms_per_launch);
float goicp_rot_coeff(goicp_handle h, int32_t level);
float goicp_trans_delta(float child_width);
/* angle-axis vector (a rotation-cube centre) -> rotation matrix, float arithmetic in the order of
 * GoICP::OuterBnB (src/goicp/jly_goicp.cpp:449-467); host-side helper */
void goicp_rodrigues(const float v[3], float R[9]);

/* Registration::compute_sse_error(glm::mat3 R, glm::vec3 t) (src/fgoicp/registration.hpp:96) scored
 * with the DT as GoICP::ICP does (src/goicp/jly_goicp.cpp:100-129). */
int goicp_eval_sse(goicp_handle h, const float R[9], const float t[3], float* sse);

/* FastGoICP::branch_and_bound_R3(rnode, fix_rot) (src/fgoicp/fgoicp.cpp:107-181) == GoICP::InnerBnB
 * (src/goicp/jly_goicp.cpp:227-340).  best_node = {corner x,y,z, width}, written only on improvement. */
typedef struct goicp_counters {
	int64_t rot_pops, trans_pops, cubes, inner_calls, icp_runs, icp_iters, bounds_launches;
	int64_t queue_fallbacks;     /* batches of inner searches in which a device queue outgrew its slab: the searches concerned (only they, since round 4)
	                              * were re-run through the host queues */
	int64_t tile_expansions;     /* BnB expansions (8 cube bounds each, counted in `cubes` too) evaluated from LDS-staged DT tiles */
	int64_t lane_batches;        /* batches of inner searches cut into two or more lanes (goicp_params::lanes) */
} goicp_counters;
int goicp_inner_bnb(goicp_handle h, const float R[9], int32_t level, float incumbent, float* value,
                    float best_node[4], goicp_counters* counters);

/* IterativeClosestPoint3D::run (src/fgoicp/icp3d.hpp:30-35, icp3d.cu:83-108) == ICP3D<float>::Run
 * (src/goicp/jly_icp3d.hpp:181-295).  R,t in/out; err = sum of squared NN distances of the last pass. */
int goicp_icp_run(goicp_handle h, float R[9], float t[3], int32_t max_iter, float err_diff,
                  float* err, int32_t* iters);
/* K independent ICP3D<float>::Run loops on one handle, one start pose each, refined together in one device loop (multi-start ICP: the
 * candidates of a coarse search, the symmetric poses of an object, detector or RANSAC hypotheses).  R: K x 9, t: K x 3, row-major, in/out.
 * err (K, may be NULL): sum of squared NN distances of each pose's last pass.  iters (K, may be NULL): each pose's iteration count.
 * Pose k's result is bit-identical to goicp_icp_run(h, R + 9k, t + 3k, max_iter, err_diff, ...) on the same handle, under the handle's ICP
 * options (goicp_set_icp_options: metric 0 and 1).  goicp_cancel stops it as it stops goicp_icp_run; the counters add icp_runs += K and
 * icp_iters += the passes of all poses.  The handle's single-pose ICP state, the goicp_icp_step pose, the goicp_poll snapshot and the
 * neighbour cache are left alone.  GOICP_ERR_INVALID: K == 0 or K > 1024, a NULL h, R or t, max_iter < 0, trim_fraction > 0, metric 0
 * without goicp_icp_run's fixed-point pass (dt_layout = 0 or icp_fused = 1), a registration running on the handle. */
int goicp_icp_run_batch(goicp_handle h, size_t K, float* R, float* t, int32_t max_iter, float err_diff,
                        float* err, int32_t* iters);
/* average duration (ms) of one ICP correspondence pass (NN + sums) at the given pose */
int goicp_time_icp_pass(goicp_handle h, const float R[9], const float t[3], int32_t iters, float* ms_per_pass);
/* the same with the neighbour cache in play at a repeated pose: every query hits (the steady-state floor of a pass);
 * goicp_time_icp_pass itself bypasses the cache: every query walks the tree (a pass at a new pose) */
int goicp_time_icp_pass_cached(goicp_handle h, const float R[9], const float t[3], int32_t iters, float* ms_per_pass);

/* kernKDSearchNearest (src/icp_kernel.cu:146-157) / kernFindNearestNeighbor (src/fgoicp/icp3d.cu:13-30):
 * exact 1-NN of n query points in the target; ties -> lowest target index. */
int goicp_nn_query(goicp_handle h, const float* query_xyz, size_t n, int32_t* index, float* dist_sq);

/* ---- point-to-plane ICP (opt-in; new, the reference has point-to-point only) ---------------------------------------------
 * The options apply to every ICP the handle runs: goicp_icp_run, goicp_icp_step, goicp_time_icp_pass (it times the pass of the chosen
 * metric), the ICP inside goicp_register (every driver) and the per-rank ICP of goicp_register_sharded*.  With metric 1 every iteration
 * is one damped Gauss-Newton step on sum_i ((q_i - m_i) . n_i)^2, linearised about the transformed source centroid: m_i = the exact
 * nearest target point of q_i (the same neighbour search as point-to-point), n_i = its normal.  err keeps its meaning: the sum of
 * squared NN distances of the last pass; the stop rule is ICP3D::Run's.  Where the 6x6 matrix of an iteration is rank deficient under
 * goicp_pose_information's default rule (eigenvalues <= 1e-6 of the largest; a planar target: rank 3), the step is the minimum-norm one
 * over the retained eigenvalues: no motion along a direction the correspondences leave free.  Refused (GOICP_ERR_INVALID): metric 1 with trim_fraction > 0,
 * metric outside {0, 1}, normal_k outside [3, 32], any change while a registration runs.  goicp_icp_run_collective runs metric 1
 * replicated on every rank (the metric joins its check word); goicp_register_multi_gpu stays point-to-point. */
typedef struct goicp_icp_options {
	int32_t metric;     /* 0 point-to-point = ICP3D<float>::Run (default), 1 point-to-plane */
	int32_t normal_k;   /* neighbours per target normal (the point itself included), 3..32, default 16 */
} goicp_icp_options;
void goicp_icp_options_default(goicp_icp_options* out);
/* builds the target normals when metric == 1 (once per normal_k): k-NN, fp64 covariance, eigenvector of the smallest eigenvalue,
 * oriented so that n . (p - target centroid) >= 0 (a zero product: first nonzero component positive); degenerate neighbourhoods get 0 */
int goicp_set_icp_options(goicp_handle h, const goicp_icp_options* opt);
/* exact k nearest target points of n queries, ascending (dist_sq, index); 1 <= k <= min(32, M) else GOICP_ERR_INVALID.
 * index / dist_sq: n x k.  k = 1 gives goicp_nn_query's result bit for bit. */
int goicp_knn_query(goicp_handle h, const float* query_xyz, size_t n, int32_t k, int32_t* index, float* dist_sq);
/* the target normals (M x 3, original target order) with the handle's normal_k; built on first use if needed */
int goicp_target_normals(goicp_handle h, float* normals_xyz);

/* ---- symmetric point-to-plane ICP (opt-in; a per-handle modifier of metric 1, not a metric value of its own) ---------------------
 * The objective of Rusinkiewicz, "A Symmetric Objective Function for ICP" (SIGGRAPH 2019; PCL's
 * TransformationEstimationSymmetricPointToPlaneLLS) in the incremental form of the point-to-plane iteration above: it reads the normals of
 * BOTH clouds and is exact for pairs of points on any locally quadratic surface, not only on planes.  The flag takes effect wherever
 * metric 1 is evaluated on the handle -- goicp_icp_run, _step, _run_batch, goicp_time_icp_pass, the refinements of goicp_register (every
 * driver) and of goicp_register_sharded*, goicp_pose_information[_batch] with metric -1 or 1 -- and is stored and inert under metric 0; a
 * handle that never sets it runs none of this.  For a correspondence with q = R p + t (the engine's float expression), m the nearest
 * target point (the unchanged walk: same index, same d^2 bits), nm = the target normal of m and ns = the source normal of p, in float,
 * left to right, without contraction:
 *   s   = R ns                       by the row expression of q without t;
 *   dot = s.x nm.x + s.y nm.y + s.z nm.z;  dot < 0: s = -s   ("enforce same direction": the objective does not depend on either
 *                                          cloud's orientation convention);
 *   n   = 0.5f * (s + nm);           s exactly zero: n = nm; nm exactly zero: n = s; both: n = 0 (the correspondence adds only d^2);
 *                                    |n| <= 1;
 *   e = q - m,  a = q - cq,  c = a - 0.5f * e    (the midpoint of the correspondence relative to the pivot cq); s exactly zero:
 *                                    c = a, so the correspondence is plain point-to-plane, bit for bit;
 *   r = e . n,  J = (c x n, n).
 * Everything after J and r is point-to-plane's: the 21 + 6 + 1 sums, the 64-bit fixed-point replicas, the damped Cholesky step, the pose
 * and pivot update, ICP3D::Run's stop rule on sum d^2, the gate's inlier word, the robust weight of |r| with rho of d.
 * Source normals: estimated on the device on first use (or as part of a source swap while the flag is on and metric 1 is active) --
 * goicp_estimate_normals of the handle's source cloud (the N points it registers) with k = source_normal_k and no viewpoint -- or the
 * caller's own (goicp_set_source_normals).  Every source swap (goicp_set_source, _voxel, _filtered, _pipeline, _clustered) drops both; a
 * swap to fewer than source_normal_k points is refused while the flag is on, before anything on the handle changes.
 * All four calls refuse with GOICP_ERR_INVALID, and change nothing: a NULL argument, source_normal_k outside 3..32 or above the source's
 * size, enabled together with trim_fraction > 0 or with a gate whose min_inliers is below 6, any call while a registration runs.
 * goicp_icp_run_collective runs the symmetric form replicated on every rank (the flag and source_normal_k join its check word);
 * goicp_register_multi_gpu stays point-to-point. */
int goicp_set_icp_symmetric(goicp_handle h, int32_t enabled, int32_t source_normal_k);
int goicp_get_icp_symmetric(goicp_handle h, int32_t* enabled, int32_t* source_normal_k, int32_t* user_normals);
/* the source normals (N x 3, original source order) the symmetric form reads: the estimated ones (built on first use) or the caller's */
int goicp_source_normals(goicp_handle h, float* normals_xyz);
/* the caller's own normals (e.g. a sensor's), original source order; they take the estimated ones' place until the next source swap.
 * n must be the handle's source count; every value finite; each normal exactly zero or of length within 1e-3 of 1 (checked in fp64),
 * stored as given */
int goicp_set_source_normals(goicp_handle h, const float* normals_xyz, size_t n);

/* ---- generalized (plane-to-plane) ICP (opt-in; the other per-handle modifier of metric 1, not a metric value of its own) -----------
 * Generalized-ICP (Segal, Haehnel, Thrun, RSS 2009) in its plane-to-plane version -- PCL's GeneralizedIterativeClosestPoint, Open3D's
 * registration_generalized_icp -- in the incremental form of the point-to-plane iteration above.  Each cloud's local surface covariance
 * has the eigenvalues (1, 1, epsilon) about the point's normal n, C = I - (1 - epsilon) n n^T, a function of the normal alone, and a
 * correspondence is weighted by the inverse of the two covariances' sum.  goicp_set_icp_options(2, ..), (3, ..) and
 * goicp_pose_information(metric = 2) stay refused; no struct changes size; goicp_abi_version() stays 4.  The flag takes effect wherever
 * metric 1 is evaluated on the handle -- goicp_icp_run, _step, _run_batch, goicp_time_icp_pass, the refinements of goicp_register (every
 * driver) and of goicp_register_sharded*, goicp_pose_information[_batch] and goicp_result_information with metric -1 or 1 -- and is
 * stored and inert under metric 0; a handle that never sets it runs none of this.  For a correspondence with q = R p + t (the engine's
 * float expression), m the nearest target point (the unchanged walk: same index, same d^2 bits), u = the target normal of m and
 * ns = the source normal of p, e = q - m and a = q - cq (cq the pivot) -- in float, every sum left to right as written, without
 * contraction, `/` the correctly rounded division:
 *   s   = R ns                       by the row expression of q without t (the symmetric form's);
 *   k   = 1 - epsilon,  h = 2 * epsilon;
 *   Sigma = 2 I - k (u u^T + s s^T), its six unique entries:
 *     Sxx = 2 - k * (u.x * u.x + s.x * s.x)      Syy, Szz likewise;
 *     Sxy = -(k * (u.x * u.y + s.x * s.y))       Sxz, Syz likewise.
 *     A normal that is exactly zero adds exact zeros, so that point's covariance is I; no product sees a normal's sign;
 *   the cofactors  C00 = Syy * Szz - Syz * Syz   C01 = Sxz * Syz - Sxy * Szz   C02 = Sxy * Syz - Sxz * Syy
 *                  C11 = Sxx * Szz - Sxz * Sxz   C12 = Sxy * Sxz - Sxx * Syz   C22 = Sxx * Syy - Sxy * Sxy
 *   det = Sxx * C00 + Sxy * C01 + Sxz * C02;
 *   W   = 2 epsilon Sigma^-1:  Wij = (h * Cij) / det.   Sigma's eigenvalues lie in [2 epsilon, 2], so W's lie in [epsilon, 1]: the
 *         minimiser is that of sum e^T Sigma^-1 e, and every summed term keeps point-to-plane's bound (|n| <= 1 there).
 *         epsilon = 1: W = I exactly (point-to-point Gauss-Newton about the pivot); both normals zero: W = epsilon I exactly;
 *   g   = W e:   g.x = W00 * e.x + W01 * e.y + W02 * e.z   (rows of the symmetric W likewise);
 *   the system linearised with e' = e + omega x a + tau:
 *     right-hand side  b = (a x g, g),   a x g = (a.y * g.z - a.z * g.y, a.z * g.x - a.x * g.z, a.x * g.y - a.y * g.x);
 *     M = [a]x W, row i the i-th component of a x (column j of W):  M0j = a.y * W2j - a.z * W1j,  M1j = a.z * W0j - a.x * W2j,
 *                                                                    M2j = a.x * W1j - a.y * W0j;
 *     H_tt = W,  H_wt = M,  H_ww = M [a]x^T:  Hi0 = Mi2 * a.y - Mi1 * a.z,  Hi1 = Mi0 * a.z - Mi2 * a.x,  Hi2 = Mi1 * a.x - Mi0 * a.y;
 *     the 21 words are the upper triangle of [[H_ww, H_wt], [., H_tt]] in point-to-plane's J J^T order, the 28th word is d^2.
 * Everything after these 28 words is point-to-plane's: the 64-bit fixed-point replicas, the damped fp64 Cholesky step, the pose and pivot
 * update, ICP3D::Run's stop rule on sum d^2 (err keeps its meaning), the gate's inlier word.  Under a robust kernel
 * (goicp_set_icp_robust) the weight is taken of the Euclidean distance d = sqrt(d^2) -- metric 0's argument: the residual here is a
 * vector -- it multiplies the 27 terms in the column sums, and rho of d goes to the cost.  goicp_pose_information reports sum w e^T W e
 * where point-to-plane reports sum w r^2.
 * epsilon must lie in [1e-4, 1]; the default is 1e-3, PCL's gicp_epsilon and Open3D's.  source_normal_k (3..32, at most N) and the
 * source normals are the symmetric flag's: goicp_source_normals and goicp_set_source_normals serve both flags -- built on first use,
 * rebuilt inside every source swap (goicp_set_source, _voxel, _filtered, _pipeline, _clustered, _segmented) while a flag is on and
 * metric 1 is active, dropped at every swap otherwise; a swap to fewer than source_normal_k points is refused before anything changes.
 * Refused with GOICP_ERR_INVALID, changing nothing: a NULL argument, epsilon or source_normal_k out of range, enabled together with
 * trim_fraction > 0 or with a gate whose min_inliers is below 6, any call while a registration runs, enabled while the symmetric flag
 * is on -- and goicp_set_icp_symmetric(1, ..) while this flag is on.  goicp_icp_run_collective runs the form replicated on every rank
 * (the flag, epsilon's bits and source_normal_k join its check word); goicp_register_multi_gpu stays point-to-point. */
int goicp_set_icp_generalized(goicp_handle h, int32_t enabled, float epsilon, int32_t source_normal_k);
int goicp_get_icp_generalized(goicp_handle h, int32_t* enabled, float* epsilon, int32_t* source_normal_k, int32_t* user_normals);

/* ---- distance-gated ICP (opt-in; new: a maximum correspondence distance, the outlier rule of PCL / Open3D) ----------------------
 * The gate applies to every ICP the handle runs, both metrics: goicp_icp_run, goicp_icp_run_batch, goicp_icp_step, goicp_time_icp_pass, the
 * ICP inside goicp_register (every driver) and the per-rank ICP of goicp_register_sharded* (the DT re-score of a refined pose still scores
 * all N points, so the search's guarantee is untouched).  g = max_corr_dist, in cloud units as handed to goicp_create; g2 = g * g in float.
 *   - a correspondence is an inlier iff d^2 <= g2, d^2 being the float goicp_nn_query returns for the transformed point (ties and
 *     neighbours are goicp_nn_query's): the inlier set of a pass depends on the pose only;
 *   - all sums of an iteration run over the inliers, n_in of them; the update is the ungated one with n_in in place of n;
 *   - err = the inliers' sum of d^2 of the last pass; goicp_icp_inliers = its n_in;
 *   - stop rule: ICP3D::Run's one-sided test on the truncated cost C = err + (N - n_in) * g2 (= sum of min(d^2, g2)):
 *     stop iff C_prev > 0 && C_prev - C_new < err_diff * N;
 *   - n_in < min_inliers: the pose stays and the loop stops, status GOICP_OK;
 *   - while no pass rejects a point, R, t, err and iters are those of the ungated run, bit for bit.
 * Refused (GOICP_ERR_INVALID): a negative, NaN or infinite distance, min_inliers below the metric's floor (3 point-to-point, 6
 * point-to-plane; 0 = that floor), capped_walk outside {0, 1}, a gate together with trim_fraction > 0, with dt_layout = 0 or with
 * icp_fused = 1 (the gated pass is fixed-point only), any change while a registration runs.  icp_nn_cache is ignored under a gate (every
 * query walks).  goicp_icp_run_collective: the gate joins the check word and the loop runs replicated on every rank;
 * goicp_register_multi_gpu stays ungated. */
typedef struct goicp_icp_gate {
	float max_corr_dist;   /* 0 = off (default) */
	int32_t min_inliers;   /* 0 = the metric's default */
	int32_t capped_walk;   /* 1 (default): the neighbour walk prunes at g2 -- same inliers, same sums; 0: the full walk */
} goicp_icp_gate;
void goicp_icp_gate_default(goicp_icp_gate* out);
int goicp_set_icp_gate(goicp_handle h, const goicp_icp_gate* gate);
/* inlier counts of the last goicp_icp_run (K = 1) or goicp_icp_run_batch (its K); without a gate every count is N.  Any other K: GOICP_ERR_INVALID */
int goicp_icp_inliers(goicp_handle h, size_t K, int32_t* inliers);
/* the correspondences of the source cloud at R|t, one launch: per source point (original order) the neighbour's target index (-1 when
 * d^2 > max_corr_dist^2) and d^2 -- the bits an ICP pass at this pose sees (same transform expression, same walk) -- plus the inlier count
 * and the inliers' sum of d^2 (summed in double in source order, rounded once).  max_corr_dist = 0: no gate.  Any output may be NULL. */
int goicp_eval_correspondences(goicp_handle h, const float R[9], const float t[3], float max_corr_dist,
                               int32_t* index, float* dist_sq, int32_t* inliers, float* sse_inliers);

/* ---- robust-kernel ICP (opt-in; new: M-estimator weights, the RobustKernel of Open3D / the loss functions of Ceres) ---------------
 * Iteratively re-weighted least squares: every correspondence is weighted smoothly by its residual.  The kernel applies to every ICP the
 * handle runs, both metrics, exactly where the gate does: goicp_icp_run, goicp_icp_run_batch, goicp_icp_step, goicp_time_icp_pass, the ICP
 * inside goicp_register (every driver) and the per-rank ICP of goicp_register_sharded* (the DT re-score of a refined pose is unchanged, so
 * the search's guarantee is untouched).  c = scale, in cloud units as handed to goicp_create; d = sqrtf(d^2), d^2 being the float
 * goicp_nn_query returns for the transformed point; the residual is r = d (metric 0) or r = |(q - m) . n| (metric 1); u = r / c, v = d / c.
 *   kernel             weight w(r)                        cost term rho
 *   1 Huber            1 if r <= c, else c / r            d^2 if d <= c, else 2 c d - c^2
 *   2 Cauchy           1 / (1 + u^2)                      c^2 log1p(v^2)
 *   3 Geman-McClure    1 / (1 + u^2)^2                    d^2 / (1 + v^2)
 *   4 Tukey            (1 - u^2)^2 if r <= c, else 0      c^2/3 (1 - (1 - v^2)^3) if d <= c, else c^2/3
 *   - every term an iteration sums (metric 0: the 15 Kabsch terms; metric 1: the 27 terms of J J^T and J r) is multiplied by w in float;
 *     the update is the plain one with W = sum w in place of n (carried means included; metric 1: the same damped system, weighted);
 *   - err keeps its meaning: the sum of d^2 over ALL N points of the last pass;
 *   - stop rule: ICP3D::Run's one-sided test on the robust cost C = sum rho: stop iff C_prev > 0 && C_prev - C_new < err_diff * N.  rho is
 *     taken of the distance d for both metrics -- for metric 0 that is rho(r); for metric 1 it is the robust form of the sum of d^2 that the
 *     plain point-to-plane loop tests;
 *   - W < 3 (metric 0) / 6 (metric 1): the pose stays and the loop stops, status GOICP_OK -- a redescending kernel with a scale far below
 *     the residuals ends like this; goicp_icp_robust_stats shows it;
 *   - while every weight of every pass is exactly 1 (a Huber scale above every residual), R, t, err and iters are those of the plain run,
 *     bit for bit.
 * Refused (GOICP_ERR_INVALID): a kernel outside 0..4, a scale that is <= 0, NaN or infinite with kernel != 0, a kernel together with
 * trim_fraction > 0, with a gate (in either order of setting), with dt_layout = 0 or with icp_fused = 1 (the robust pass is fixed-point
 * only), any change while a registration runs.  icp_nn_cache is ignored under a kernel (every query walks).  goicp_icp_run_collective:
 * kernel and scale join the check word and the loop runs replicated on every rank; goicp_register_multi_gpu stays plain. */
typedef struct goicp_icp_robust { int32_t kernel; float scale; } goicp_icp_robust;   /* kernel 0 = off (default) */
void goicp_icp_robust_default(goicp_icp_robust* out);
int goicp_set_icp_robust(goicp_handle h, const goicp_icp_robust* r);
/* of the last goicp_icp_run (K = 1) or goicp_icp_run_batch (its K): robust cost C and weight sum W of each pose's last pass (without a
 * kernel: err and N).  Either output may be NULL.  Any other K: GOICP_ERR_INVALID */
int goicp_icp_robust_stats(goicp_handle h, size_t K, float* cost, float* weight_sum);

/* ---- truncated-cost search (opt-in; new: an outlier-robust objective for the GLOBAL part) -------------------------------------------
 * The gate, the robust kernels and point-to-plane change the refinement only; the search itself -- cube bounds, inner and outer BnB, the
 * DT re-score that decides whether a refined pose is adopted -- minimises the plain sum of squares over all N source points.  With
 * max_dist = g > 0 (cloud units as handed to goicp_create, like the gate) the handle's search minimises the TRUNCATED cost instead, the one
 * gated ICP descends:
 *     E_g(R, t) = sum_i min(DT(R p_i + t), g)^2.
 * With m = max(DT(R p + t_c) - coeff |p|, 0) the per-point clamped residual of a cube as ever (same float expression, bit for bit):
 *     upper-bound term  min(m, g)^2               lower-bound term  min(max(m - delta, 0), g)^2
 * -- the clamp comes AFTER the subtractions.  The bounds are valid because min(e, g)^2 does not decrease in e >= 0: a lower bound of a
 * residual, clamped, is a lower bound of the clamped residual.  Everything else stays: SSEThresh = mse_threshold * N, pruning, early
 * exit, a refined pose is adopted only when its (now truncated) score improves -- so the guarantee holds whatever ICP flavour refines.
 * What changes meaning on such a handle: goicp_eval_bounds* and goicp_time_bounds_device return the truncated bounds, goicp_eval_sse
 * returns E_g, goicp_inner_bnb searches E_g, best_sse of goicp_poll (and of the result files) is E_g of the best pose, and 0 <= lb <= ub
 * <= N g^2 always.  g = +huge reproduces the plain handle's bits.
 * The threshold: n_out outliers contribute a floor of about n_out g^2 that mse_threshold * N does not know about.  A threshold ABOVE
 * that floor exits early on sloppy poses; a threshold BELOW the optimum's cost never triggers the early exit and makes the engine prove
 * the optimum of E_g (to within SSEThresh).  Choose it with the floor in mind.
 * Refused (GOICP_ERR_INVALID): a negative, NaN or infinite distance, truncation together with trim_fraction > 0 (the trimmed bounds have
 * no truncated form), any change while a registration runs.  max_dist = 0 switches truncation off again (the plain bits return).
 * goicp_register_sharded*: works when EVERY rank's handle carries the same max_dist -- as with the other per-handle options that is the
 * caller's duty, the protocol does not check it; goicp_register_multi_gpu creates its own engines and stays untruncated. */
int goicp_set_search_truncation(goicp_handle h, float max_dist);
int goicp_search_truncation(goicp_handle h, float* max_dist);

/* ---- pose information (opt-in; new: how well the data determines a pose -- the information matrix of Open3D's
 * get_information_matrix_from_point_clouds, the covariance estimators of PCL) -----------------------------------------------------
 * At a GIVEN pose R|t the Gauss-Newton normal matrix A and gradient b of the handle's ICP objective, for either metric, and their
 * finishing step.  q_i = R p_i + t (the pass's float expression: goicp_transform_source's bits), m_i its exact nearest target point and
 * d_i^2 the walk's bits (goicp_eval_correspondences'), n_i the normal of m_i (metric 1; built on first use).  Weight w_i: 1 on a plain
 * handle, [d_i^2 <= g2] under the handle's gate, the handle's robust kernel weight (same float arithmetic as the robust pass) under a
 * kernel.  Pivot c: the caller's, by default R src_centroid + t.  With a_i = q_i - c the perturbation is q' = Exp(omega)(q - c) + c + tau,
 * x = (omega, tau):
 *   metric 0: e = q - m, J = [ -[a]x | I ]:  A = sum w J^T J, b = sum w J^T e = (sum w a x e, sum w e), cost = sum w d^2, dim = 3
 *   metric 1: j = (a x n, n), r = e . n:     A = sum w j j^T, b = sum w j r,                           cost = sum w r^2, dim = 1
 * sse = sum d^2 over ALL N points, weight_sum W = sum w, inliers = the points with w > 0.  The sums are float per workgroup, then exact
 * 64-bit fixed point: the result does not depend on the order workgroups arrive in.  Finishing step, fp64 on the host: eigenvalues
 * (ascending) and eigenvectors (rows) of A by cyclic Jacobi; rank = the eigenvalues > rank_tol * lambda_max; dof = dim W - 6;
 * sigma2 = cost / dof and covariance = sigma2 * pinv A over the retained eigenvalues when dof > 0; else sigma2 = 0, covariance = 0 and
 * dof_nonpositive = 1 (status still GOICP_OK).  This is the Gauss-Newton / Cramer-Rao covariance for FIXED correspondences with i.i.d.
 * residuals; it ignores correspondence uncertainty (it is not Censi's estimator).
 * Refused (GOICP_ERR_INVALID): trim_fraction > 0, dt_layout = 0 or icp_fused = 1 (the pass is fixed-point only, as the gate), a metric
 * outside {-1, 0, 1}, a non-finite R, t or pivot, a pivot so far away that the fixed-point sums would overflow, rank_tol outside [0, 1),
 * K outside 1..1024, any call while a registration runs.  A handle that never calls these launches what it launched before. */
typedef struct goicp_pose_info_options {
	int32_t metric;      /* -1 = the handle's (default), 0 point-to-point, 1 point-to-plane */
	int32_t use_pivot;   /* 0 (default): the transformed source centroid; 1: pivot[] */
	double pivot[3];
	double rank_tol;     /* default 1e-6: the terms are float, 2^-24 per rounding, so an eigenvalue below ~16 roundings of the largest is
	                        indistinguishable from zero */
} goicp_pose_info_options;
void goicp_pose_info_options_default(goicp_pose_info_options* out);
typedef struct goicp_pose_info {
	double information[36];   /* A, row-major, omega then tau */
	double gradient[6];       /* b */
	double covariance[36];
	double eigenvalues[6];    /* ascending */
	double eigenvectors[36];  /* row i belongs to eigenvalues[i] */
	double pivot[3];          /* the pivot used (as the float the pass subtracted) */
	double weight_sum, cost, sse, sigma2;
	int64_t inliers;
	int32_t rank, metric, dof_nonpositive;
} goicp_pose_info;
/* opt = NULL: the defaults */
int goicp_pose_information(goicp_handle h, const float R[9], const float t[3], const goicp_pose_info_options* opt, goicp_pose_info* out);
/* K poses (R: K x 9, t: K x 3) in one launch, out[K]; slot k is the single call at pose k bit for bit */
int goicp_pose_information_batch(goicp_handle h, size_t K, const float* R, const float* t, const goicp_pose_info_options* opt,
                                 goicp_pose_info* out);
/* the same at optR | optT of the handle's last finished registration; GOICP_ERR_INVALID when there is none */
int goicp_result_information(goicp_handle h, const goicp_pose_info_options* opt, goicp_pose_info* out);
/* the finishing step on its own (host only, no handle, no GPU): info is symmetrised as (A + A^T) / 2; eig ascending, vec rows, pinv over
 * the eigenvalues > rank_tol * lambda_max (an eigenvalue exactly AT the threshold is dropped).  Any output may be NULL.
 * GOICP_ERR_INVALID: a non-finite entry, rank_tol outside [0, 1) */
int goicp_information_decompose(const double info[36], double rank_tol, double eig[6], double vec[36], double pinv[36], int32_t* rank);

/* ICP::kdTreeGPUStep / ICP::naiveGPUStep (src/icp_kernel.h:9-13, icp_kernel.cu:176-279): ONE ICP
 * iteration from the engine's current step pose (identity after create); the accumulated pose is
 * visible through goicp_poll().curR/curT. */
int goicp_icp_step(goicp_handle h);

/* FastGoICP::run() (src/fgoicp/fgoicp.cpp:9-30) == GoICP::Register() (src/goicp/jly_goicp.cpp:569-585).
 * Blocking; intended for a worker thread. */
int goicp_register(goicp_handle h);
int goicp_cancel(goicp_handle h);      /* the reference's global `goicp_finished` flag (src/goicp/jly_goicp.cpp:400) */

/* Result API: FastGoICP::{get_best_error(), optR, optT, curR, curT, finished} (src/fgoicp/fgoicp.hpp:34,67-69),
 * read by ICP::goicpGPUStep (src/goicp_kernel.cu:161-177).  A consistent snapshot; thread-safe. */
typedef struct goicp_result {
	float optR[9], optT[3];
	float curR[9], curT[3];
	float best_sse;
	int32_t finished;
	goicp_counters counters;
	double dt_build_ms, register_ms;
} goicp_result;
int goicp_poll(goicp_handle h, goicp_result* out);
/* Progress callback: invoked on the registering thread after every published snapshot (new best pose, end of a
 * rotation round, finish).  This is how the C++ shim keeps FastGoICP::{optR,optT,curR,curT,finished} current while
 * run() is executing on a worker thread (the reference's worker writes those members itself,
 * src/fgoicp/fgoicp.cpp:68-69,85-86).  cb = NULL clears it.  Not to be changed while goicp_register() runs. */
typedef void (*goicp_progress_fn)(const goicp_result* snapshot, void* user);
int goicp_set_progress_callback(goicp_handle h, goicp_progress_fn cb, void* user);
/* the output.toml the reference's configs promise (test/bunny_goicp.toml:12) but never write */
int goicp_result_write_toml(goicp_handle h, const char* path);
/* the viz.ply the reference's configs promise (test/bunny_goicp.toml:13) but never write: binary
 * little-endian PLY, target points (grey) followed by the source under optR|optT (red) */
int goicp_result_write_ply(goicp_handle h, const char* path);
/* source cloud under (R,t), original point order (what src/goicp_kernel.cu:181-193 draws) */
int goicp_transform_source(goicp_handle h, const float R[9], const float t[3], float* out_xyz);

/* ---- multi-GPU: rotation cubes sharded over ranks (new; the reference is single-GPU) -----------
 * Each rank owns every world-th cube of the 64 level-2 rotation cubes and runs its own best-first
 * search; between steps the caller min-all-reduces best_sse (and broadcasts the winner's R|t) and
 * feeds the result back with goicp_offer_best(). */
typedef struct goicp_step_status {
	int32_t finished, early_exit;
	float best_sse, frontier_lb;
	int64_t rot_pops;
} goicp_step_status;
int goicp_set_shard(goicp_handle h, int32_t rank, int32_t world);
int goicp_register_begin(goicp_handle h);
int goicp_register_step(goicp_handle h, int32_t max_rot_pops, goicp_step_status* out);
int goicp_offer_best(goicp_handle h, float sse, const float R[9], const float t[3]);
int goicp_register_end(goicp_handle h);

/* ---- the sharded registration inside the library (csrc/shard.cpp, csrc/rccl_comm.cpp) ------------------------------
 * One call per rank drives the whole protocol: step the local search, ONE all-reduce(MIN) of six packed 64-bit words
 * per step ({best SSE, rank}, frontier lower bound, early-exit / active / idle flags, failure word), a 48-byte broadcast
 * of the winner's R|t only when the global best moved, global termination, and -- when a rank runs dry -- rebalancing
 * (queue sizes gathered, every second cube of the largest queue broadcast to the idle rank).
 * Failure is a collective decision: a rank whose engine callback fails keeps taking part in the exchange, every rank
 * leaves the loop in the same iteration, ends its registration and returns an error (its own status, or GOICP_ERR_PEER
 * with goicp_shard_stats.failed_rank set).  A collective that misses the communicator's deadline returns
 * GOICP_ERR_TIMEOUT on the rank that waited.
 * The communicator is a callback table, so the protocol also runs (and is tested) without RCCL. */
typedef struct goicp_comm_ops {
	void* ctx;
	int32_t rank, world;
	/* element-wise MIN over the ranks of n unsigned 64-bit words, in place; blocking */
	int (*allreduce_min_u64)(void* ctx, uint64_t* words, size_t n);
	/* broadcast `bytes` bytes from rank `root`; blocking */
	int (*bcast)(void* ctx, void* buf, size_t bytes, int32_t root);
} goicp_comm_ops;
typedef struct goicp_shard_stats {
	int64_t steps, exchanges, broadcasts, donations, donated_cubes;
	int64_t steps_idle;   /* steps in which this rank had nothing left to expand while the search went on */
	double wait_ms;       /* host time this rank spent blocked in collectives (waiting for the slowest rank) */
	double step_ms;       /* host time inside the engine's step() */
	float best_sse;
	int32_t failed_rank;  /* -1, or the rank whose failure ended the run */
} goicp_shard_stats;
typedef struct goicp_shard_options {
	int32_t rot_pops_per_step;  /* rotation parents per step (>= 1); with ramp_to: of the FIRST step */
	int32_t rebalance;          /* 1: idle ranks receive cubes from the largest queue */
	int32_t stale_exchange;     /* 0: the exchange of a step is consumed before the next step (bulk-synchronous);
	                               1: it runs on a helper thread while the next step is evaluated and is consumed after it --
	                               a rank waits only for ranks more than one step behind */
	int32_t ramp_to;            /* 0: every step expands rot_pops_per_step parents.  R > rot_pops_per_step: the step width doubles
	                               from step to step up to R -- the single-GPU driver's own ramp (8, 16, 32, 64 rotation parents per
	                               batch: few, large launches once a registration has proved to be long), one exchange per batch.
	                               (This field was `reserved`, always 0, up to ABI 3.) */
} goicp_shard_options;
/* the engine side of the protocol as a callback table (goicp_register_sharded fills it for a real engine; tests
 * supply a CPU stand-in).  nodes7: 7 floats per rotation cube {corner x,y,z, width, ub, lb, level}. */
typedef struct goicp_shard_engine_ops {
	void* ctx;
	float sse_threshold;
	int (*begin)(void* ctx, int32_t rank, int32_t world);
	int (*step)(void* ctx, int32_t max_rot_pops, goicp_step_status* out);
	int (*pose)(void* ctx, float* sse, float R[9], float t[3]);
	int (*offer)(void* ctx, float sse, const float R[9], const float t[3]);
	int (*queue_size)(void* ctx, int32_t* n);
	int (*donate)(void* ctx, int32_t max_nodes, float* nodes7, int32_t* n);
	int (*receive)(void* ctx, const float* nodes7, int32_t n);
	int (*end)(void* ctx);
} goicp_shard_engine_ops;
int goicp_run_sharded(const goicp_shard_engine_ops* engine, const goicp_comm_ops* comm, int32_t rot_pops_per_step,
                      int32_t rebalance, goicp_shard_stats* stats);
/* the same for an engine handle (blocking; one call per rank, each rank with its own engine on its own GPU) */
int goicp_register_sharded(goicp_handle h, const goicp_comm_ops* comm, int32_t rot_pops_per_step, int32_t rebalance,
                           goicp_shard_stats* stats);
/* both with the full option set */
void goicp_shard_options_default(goicp_shard_options* out);   /* 8 parents in the first step, ramp_to 32, rebalancing on, bulk-synchronous */
int goicp_run_sharded_opt(const goicp_shard_engine_ops* engine, const goicp_comm_ops* comm, const goicp_shard_options* opt,
                          goicp_shard_stats* stats);
int goicp_register_sharded_opt(goicp_handle h, const goicp_comm_ops* comm, const goicp_shard_options* opt, goicp_shard_stats* stats);
/* element-wise SUM over the ranks of n signed 64-bit words, wrapping mod 2^64, in place; blocking, under the communicator's deadline
 * (GOICP_ERR_TIMEOUT like the other collectives).  A communicator of this library sums natively (thread: a rendezvous; RCCL:
 * ncclAllReduce(ncclInt64, ncclSum) on its own stream); any other table falls back to `world` broadcasts of the n words, added up on
 * every rank -- the same totals everywhere. */
int goicp_comm_allreduce_sum_i64(const goicp_comm_ops* comm, int64_t* words, size_t n);
/* ICP3D<float>::Run (src/goicp/jly_icp3d.hpp:181-295) with the source points sharded over the ranks -- the semantics of goicp_icp_run,
 * every rank ending with its world-1 result bit for bit (R, t, err, iters).  Every rank calls it with the same arguments and an engine
 * made from the same clouds and parameters.  Rank r of G evaluates the workgroups [floor(r B / G), floor((r+1) B / G)) of the world-1
 * grid of the fixed-point ICP pass (B workgroups of 16 queries: the same queries per workgroup as at world 1, so the same float row
 * sums) and the ranks add up the 16 integer totals per iteration (goicp_comm_allreduce_sum_i64); every rank then runs the same update
 * on the same totals, so all agree on the pose, the error and when to stop with no further collective.  One iteration: slice pass,
 * export, read back, sum over the ranks, upload, update.  A rank whose range is empty takes part with zero totals.
 * Agreement and failure are collective: the ranks first compare a check word over (R, t, max_iter, err_diff, N, fixed-point scale)
 * -- ranks that disagree all return GOICP_ERR_INVALID, none hangs -- and every sum carries a health word: a rank whose HIP call
 * failed keeps exchanging and all ranks leave in the same iteration with their own status or GOICP_ERR_PEER.
 * Replicated fallback (every rank runs the full loop, no sums; goicp_icp_shard_stats.sliced = 0): trim_fraction > 0, icp_fused = 1,
 * dt_layout = 0 -- none of these has the fixed-point pass.  The result is still identical on all ranks. */
int goicp_icp_run_collective(goicp_handle h, const goicp_comm_ops* comm, float R[9], float t[3], int32_t max_iter, float err_diff,
                             float* err, int32_t* iters);
typedef struct goicp_icp_shard_stats {
	int32_t rank, world;
	int32_t block_begin, block_end;   /* this rank's workgroups [block_begin, block_end) of the world-1 pass grid (last run) */
	int32_t blocks;                   /* workgroups of that grid */
	int32_t sliced;                   /* last run: 1 sliced passes, 0 the replicated fallback */
	int64_t queries;                  /* source points this rank evaluated, over all passes */
	int64_t runs, passes, collectives;
	double sum_wait_ms;               /* host time blocked in the sums (waiting for the slowest rank) */
	double round_trip_ms;             /* host time of the per-iteration round trip: launch, read-back, upload */
} goicp_icp_shard_stats;
/* this engine's collective ICP runs, accumulated since goicp_create */
int goicp_icp_shard_stats_get(goicp_handle h, goicp_icp_shard_stats* out);
/* goicp_register_sharded_opt with every refinement collective: the initial ICP from the identity runs as goicp_icp_run_collective
 * inside the protocol's begin, a rank adopts an improved upper bound without refining it, and when an exchange moves the global best
 * to an unrefined pose every rank refines that pose with goicp_icp_run_collective, re-scores it with the DT and offers the result --
 * one refinement per global winner instead of one per candidate on every rank.  stale_exchange = 1 is GOICP_ERR_INVALID (its helper
 * thread would interleave collectives). */
int goicp_register_sharded_collective_icp(goicp_handle h, const goicp_comm_ops* comm, const goicp_shard_options* opt, goicp_shard_stats* stats);
/* deadline of every single collective of a communicator made by this library (thread or RCCL); default: the
 * environment's GOICP_COMM_TIMEOUT_MS, else 60 000 ms.  A collective that misses it returns GOICP_ERR_TIMEOUT and leaves
 * the communicator unusable (destroy it; an RCCL communicator the library owns is aborted with ncclCommAbort). */
int goicp_comm_set_timeout_ms(goicp_comm_ops* comm, int32_t timeout_ms);
/* in-process communicator: `world` host threads of ONE process, rank r calling with out[r] (tests; rehearsing the
 * N-rank path with N engines on one GPU).  Destroy every element. */
int goicp_thread_comm_create(int32_t world, goicp_comm_ops* out /* [world] */);
int goicp_thread_comm_destroy(goicp_comm_ops* comm);
/* RCCL communicator (ncclAllReduce / ncclBroadcast over xGMI on a stream of its own, separate from the engine's compute
 * stream).  id128: an ncclUniqueId (128 bytes) made by ONE rank with goicp_rccl_unique_id() and handed to the others
 * by whatever launched them (MPI, torch.distributed, a file); goicp_rccl_comm_create() is collective.  `device` = the
 * HIP device of this rank. */
#define GOICP_RCCL_ID_BYTES 128
int goicp_rccl_unique_id(char id128[GOICP_RCCL_ID_BYTES]);
int goicp_rccl_comm_create(const char id128[GOICP_RCCL_ID_BYTES], int32_t rank, int32_t world, int32_t device, goicp_comm_ops* out);
/* wrap an existing ncclComm_t (e.g. one of ncclCommInitAll's); the communicator stays the caller's */
int goicp_rccl_comm_wrap(void* nccl_comm, int32_t rank, int32_t world, int32_t device, goicp_comm_ops* out);
int goicp_rccl_comm_destroy(goicp_comm_ops* comm);
/* single-process form: `world` engines (one per GPU, device r for rank r) created from the same clouds and driven by
 * `world` host threads over ncclCommInitAll -- what goicp_cli --ranks N runs.  Results: rank 0's engine handle is
 * returned in *out (poll / write it like any other); stats per rank optional ([world]). */
int goicp_register_multi_gpu(const goicp_params* params, const float* target_xyz, size_t n_target, const float* source_xyz,
                             size_t n_source, int32_t world, int32_t rot_pops_per_step, goicp_handle* out, goicp_shard_stats* stats);

/* ---- measurement / test helpers ----------------------------------------------------------------
 * goicp_probe_gather: measured ceiling of the path that bounds the cube-bound kernel -- independent 4-byte loads
 * into the engine's resident distance transform, nothing else.  mode 0: the 64 lanes of a wave-instruction read 64
 * consecutive floats; mode 1: 64 different 128-byte lines; mode k in {4, 8, 16, 32}: k distinct lines per instruction, the
 * lanes in k runs of 64/k consecutive floats (the cost curve between the two extremes); mode 2: the lookups served from a
 * 64 KiB tile staged in LDS (what an LDS-staged DT tile would deliver once it is loaded; window_bytes ignored).  window_bytes = footprint each workgroup draws its
 * addresses from (rounded up to a power of two, at least 16 KiB, at most the grid).  Result: lookups per second.
 * goicp_debug_kabsch: the device-side 3x3 SVD / Kabsch routine of the ICP update (Matrix::svd use in
 * src/goicp/jly_icp3d.hpp:266-285) on a caller-supplied H (row-major), on the current device; test-only. */
int goicp_probe_gather(goicp_handle h, int32_t mode, size_t window_bytes, double* lookups_per_s);
int goicp_debug_kabsch(const float H[9], float R[9]);
/*
 * goicp_debug_bounds_tile (measurement / test): the cube bounds of the 8 children of nseg x n translation nodes (n <= 64; segment i
 * uses rotation rots9[9*i..], its nodes parents4[(i*n + e)*4..] = corner xyz + width, rotation level `level`) evaluated twice:
 * by the LDS-staged-tile kernel (north_star (a): the DT box a 64-point patch can reach under all the segment's translations is copied
 * to LDS once) and by the direct gather kernel of the search (registration.cu:27-60's role).  ub/lb arrays: 8*nseg*n floats each;
 * ms[0] / ms[1]: milliseconds per launch, tile / direct; stats[0] / stats[1]: 64-point patches staged / too large to stage.
 */
int goicp_debug_bounds_tile(goicp_handle h, const float* rots9, const float* parents4, int32_t nseg, int32_t n, int32_t level, int32_t chunks,
                            float* ub_tile, float* lb_tile, float* ub_direct, float* lb_direct, float ms[2], uint32_t stats[2]);
/*
 * goicp_debug_queue_expand (test): the n (<= 128) given translation nodes expanded by ONE round of the device-resident inner-BnB queues --
 * an upper-bound search (maxRotDisL == NULL, jly_goicp.cpp:492) and a lower-bound search (rotation level `level`, :551) of the same
 * rotation, both listing all n nodes: the lock-step round the outer search runs (bnb_queue_kernel selection + bounds_queue_kernel, the
 * twin-fused evaluation when the engine has it on).  Outputs: the 8 children's (ub, lb) of every node for both passes, in the order of
 * parents4 (inner body of GoICP::InnerBnB, jly_goicp.cpp:262-335).  info[0] = point chunks of the evaluation, info[1] = twin lists in use.
 */
int goicp_debug_queue_expand(goicp_handle h, const float R[9], int32_t level, const float* parents4, int32_t n, float* ub_ubpass, float* lb_ubpass,
                             float* ub_lbpass, float* lb_lbpass, int32_t info[2]);
/*
 * goicp_debug_queue_expand_tiles (test): goicp_debug_queue_expand with the round's TILE list on -- tile_min 1 and no spread limit, so both
 * searches list every node there and nothing in the direct list (GOICP_ERR_INTERNAL otherwise) -- evaluated by the queued LDS-tile kernel
 * (segment count and cloud split chosen on the device).  The upper-bound search queues only the first n_ub (1 <= n_ub <= n) nodes:
 * ub_ubpass / lb_ubpass hold 8 n_ub floats, ub_lbpass / lb_lbpass 8 n; with more than one point chunk the chunk partials are added on the
 * host in chunk order, in double (rounded once).  info = {point chunks, segments, workgroups of the tile launch, twin lists in use}.  GOICP_ERR_INVALID on a handle
 * without the tile list (lds_tiles 0, dt_layout 0, bounds_fp16, trimmed).
 * digest != 0: the queue kernel is launched once more (K = 1) and digests that round from the tile buffers.  queue_nodes[s][8 n][6] = the
 * queue of search s afterwards (corner xyz, width, ub, lb per node), queue_counts[s] = {nodes in it, nodes the new selection took out (0 / 1)},
 * listed4[s] = that node (corner xyz, width), search8[s] = {best, min_ub, improved, bx, by, bz, bw, done}; s = 0 upper-, 1 lower-bound search.
 */
int goicp_debug_queue_expand_tiles(goicp_handle h, const float R[9], int32_t level, const float* parents4, int32_t n, int32_t n_ub, float* ub_ubpass,
                                   float* lb_ubpass, float* ub_lbpass, float* lb_lbpass, int32_t info[4], int32_t digest, float* queue_nodes,
                                   int32_t* queue_counts, float* listed4, float* search8);
/*
 * goicp_debug_queue_round (test): ONE launch of the queue kernel (bnb_queue_kernel, csrc/bnbqueue.hip) on caller-given state and nothing
 * else -- no bound evaluation: the caller supplies the bounds of the previous round's children.  The call works on device buffers of its
 * own; of the handle it uses the device and the stream, and leaves its lanes, lists and counters alone.
 *   goicp_queue_search   the device's record of one inner search, field for field (csrc/device.hpp QSearch); in: the search before the
 *                        round (count <= cap queued nodes, n_parents <= 512 expansions of the previous round at parent_off of the previous
 *                        list, tile 0), out: the record after it.
 *   goicp_queue_round    the round: nsearch (1..8) searches = workgroups; parity (0 / 1) of the list the round writes; deep 0 / 1 = the 128- /
 *                        64-VGPR build; chunks = point chunks of the previous evaluation (1: prev_ub / prev_lb hold the children's bounds,
 *                        8 per record of the previous list; > 1: prev_scratch holds chunk partials [record][chunk][ub 8 | lb 8] and the
 *                        digest adds them); n_prev_list (<= list_cap) = records of the previous list; the other fields are QParams' of the
 *                        same names (K 1..512, cap 1..8 192, list_cap 1..65 536; root = corner xyz + width).  No tile buffers: nothing is
 *                        listed in the tile list, QSearch::deep and ctl's tile_hint still report the spread decision.
 *   nodes                [nsearch][8 192][6] floats (corner xyz, width, ub, lb); in: the first `count` nodes of every queue, out: the first
 *                        `count` nodes afterwards (the rest of a slab is not touched on the host)
 *   prev_parents         n_prev_list records {float x, y, z, w, coeff; int32 rot} (may be null when n_prev_list = 0, as prev_ub / prev_lb /
 *                        prev_scratch, of which only the one `chunks` selects is read)
 *   ctl                  in / out: {n_groups[0], n_groups[1], n_active[0], n_active[1], overflow, tile_hint} of the control block
 *   listed               out, list_cap records of the same form: the list of this round; a record the kernel did not write is all-ones bits
 *                        (NaN floats, rot -1)
 *   parent_search        out, list_cap words (-1 where not written), or null: the kernel is launched without that array
 * GOICP_ERR_INVALID, before any launch, on arguments outside these ranges.
 */
#define GOICP_QUEUE_SLAB 8192
typedef struct goicp_queue_search {
	float best, coeff;
	int32_t rot, count, done, improved, n_parents, parent_off, pops, cubes;
	float bx, by, bz, bw;
	int32_t tile;
	float min_ub;
	int32_t deep, stale, twin;
} goicp_queue_search;
typedef struct goicp_queue_round {
	int32_t nsearch, parity, deep, chunks, n_prev_list;
	float thr;
	int32_t K, kmax, cap, list_cap, soft_overflow;
	float root[4];
	int32_t boxed, depth;
	float lo[3], hi[3];
	int32_t stale_widen, stale_compact;
	float tile_spread;
	int32_t tile_min;
} goicp_queue_round;
int goicp_debug_queue_round(goicp_handle h, const goicp_queue_round* round, goicp_queue_search* searches, float* nodes, const void* prev_parents,
                            const float* prev_ub, const float* prev_lb, const float* prev_scratch, int32_t ctl[6], void* listed,
                            int32_t* parent_search);
/* goicp_debug_bounds_order (test): how the last goicp_eval_bounds_device / goicp_time_bounds_device launch of this handle walked its batch.
 * info[0] = the form launched (goicp_params::bounds_order: 0 the plain launch -- switch off, fewer groups than bounds_order_min_groups, not
 * a bricked fp32 grid in the Infinity Cache --, 1 ordered, 2 ordered + pairs); for forms 1 and 2, read back after the launch has finished:
 * info[1] = 1 when the device pre-pass built an order, 0 when it left the batch alone (more runs of equal rotation than
 * bounds_order_max_runs); info[2] = the work items of the pair list (pairs and singles; 0 when left alone) */
int goicp_debug_bounds_order(goicp_handle h, int32_t info[3]);
/* goicp_debug_bounds_twins (test): what the pair launch (form 2) of the same last call did with coincident members -- two sibling sets of
 * one item whose six translations and delta are equal bit for bit.  info[0] = items evaluated in twin form (one index set and one gather
 * per point, a sum per coefficient), info[1] = items whose coefficients were equal as well (evaluated once, stored to both).  Both 0 for the
 * other forms and for a batch the pre-pass left alone. */
int goicp_debug_bounds_twins(goicp_handle h, int32_t info[2]);
/* goicp_debug_bounds_copies (test): info[0] = the groups of the same last call that the pair launch (form 2, several point chunks,
 * bounds_dedup on) did not evaluate because their eight records repeat, bit for bit, those of another group of their run, whose sums they
 * took.  0 for the other forms, for one point chunk, for a batch the pre-pass left alone and with bounds_dedup = 0. */
int goicp_debug_bounds_copies(goicp_handle h, int32_t info[1]);
/* goicp_debug_bounds_balance (test): the mapping of the same last call.  info[0..8] = the cuts: block label x evaluated the units
 * cut[x] .. cut[x + 1] - 1 of the list u = chunk * items + item (cut[8] = 8 items); info[9..16] = lines and info[17..24] = waves of the
 * source's eight chunks (all 0 for a cloud of fewer than 7 937 points, whose cuts are the equal split); info[25] = 1 when the launch was
 * the pair form over eight chunks with bounds_balance on.  A call that was no pair launch over eight chunks reports info[25] = 0 and the
 * equal split x * items of its items. */
int goicp_debug_bounds_balance(goicp_handle h, int32_t info[26]);
/* goicp_debug_bounds_xcd_spans (diagnostic build, make -C csrc stamps): per XCC (rows 0-7) and per block label (rows 8-15) of the pair
 * launches since the last call, six 64-bit words: first workgroup entry and last exit on the 100 MHz clock, workgroups that worked, the sum of
 * their times, (XCC rows) the mask of the labels seen there, workgroups that left at once.  The call clears the stamps.
 * GOICP_ERR_INVALID in the shipped library, which stamps nothing. */
int goicp_debug_bounds_xcd_spans(goicp_handle h, uint64_t out[96]);
/* diagnostics of the ICP pass's neighbour cache: two scoring passes at (R, t); *hits = queries of the second pass that
 * skipped the tree walk (-1 when the cache is off) */
int goicp_debug_cache_hits(goicp_handle h, const float R[9], const float t[3], int64_t* hits);
/* goicp_debug_select (test): the trimmed ICP iteration's selection of the num (1 <= num <= n) smallest of d2[0..n) -- ties go to the
 * points that come first -- run on the device against a fresh (unconverged) loop state; include[i] = 1 for the selected points, else 0.
 * kernel 0: the iteration's own choice by size; 1: the register kernel (n <= 32 768, else GOICP_ERR_INVALID); 2: the streaming kernel. */
int goicp_debug_select(goicp_handle h, const float* d2, size_t n, int32_t num, int32_t kernel, uint8_t* include);
/* goicp_debug_source_order (test): the DEVICE ordering goicp_set_source uses, alone, of any finite cloud (the handle lends its device and
 * stream; its state is untouched); equals goicp_source_order_host element for element */
int goicp_debug_source_order(goicp_handle h, const float* xyz, size_t n, int32_t mode, int32_t* perm);

#ifdef __cplusplus
}
#endif
#endif /* GOICP_MI355_H */
