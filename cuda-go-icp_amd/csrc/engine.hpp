// Host side of the MI355X Go-ICP engine: owns the HBM-resident clouds / distance transform /
// k-d tree, drives the HIP kernels, and runs the branch-and-bound search and the ICP loop.
// Semantics follow the reference CPU Go-ICP path (src/goicp/jly_goicp.cpp) behind the surface of
// the reference GPU classes (src/fgoicp/fgoicp.hpp, registration.hpp, icp3d.hpp).
#pragma once
#include <atomic>
#include <cstdint>
#include <functional>
#include <mutex>
#include <queue>
#include <stdexcept>
#include <string>
#include <vector>

#include "device.hpp"
#include "hipbuf.hpp"

struct goicp_comm_ops;   // include/goicp_mi355.h
struct goicp_pose_info_options;
struct goicp_pose_info;

namespace goicp {

// a failure that already carries its goicp_status (a collective's GOICP_ERR_TIMEOUT / GOICP_ERR_PEER / GOICP_ERR_INVALID)
struct StatusError : std::runtime_error {
	int rc;
	StatusError(int code, const std::string& msg) : std::runtime_error(msg), rc(code) {}
};

// goicp_icp_shard_stats: this engine's collective ICP runs (goicp_icp_run_collective), accumulated since it was created
struct IcpShardStats {
	int rank = 0, world = 1;
	int block_begin = 0, block_end = 0, blocks = 0;   // this rank's workgroups [begin, end) of the world-1 grid of `blocks` (last run)
	int sliced = 0;                                   // last run: 1 sliced passes, 0 replicated full passes (fallback)
	long long queries = 0, runs = 0, passes = 0, collectives = 0;
	double sum_wait_ms = 0, round_trip_ms = 0;
};

struct Params {
	int dt_size = 300;            // jly_goicp.cpp:56
	double dt_expand = 2.0;       // jly_goicp.cpp:57
	float mse_threshold = 1e-3f;  // Config::mse_threshold (common.cpp:62)
	int dt_layout = 1;            // 0 linear, 1 bricked 4x4x4
	int device = -1;              // -1: current HIP device
	int trans_batch = 32;         // translation nodes expanded per inner search per launch (1 = reference order)
	int wide_children = 1;        // run the rotation children's inner searches concurrently (0 = reference order)
	int rot_batch = 64;           // most rotation nodes expanded per round when wide_children (their 8 children x {ub,lb} searches share launches); ramps up from 8
	int icp_max_iter = 10000;     // jly_icp3d.hpp:114
	int verbose = 0;
	int morton_sort = 2;          // source order on the device: 0 input order, 1 Morton curve, 2 k-d order (locality of the DT gathers)
	int icp_chunk = 16;           // ICP iterations queued per host round trip
	int kd_gpu_build = -1;        // box hierarchy built on the device (Morton sort, looser boxes): 1 yes, 0 / -1 host median splits (threaded)
	int bounds_fp16 = 0;          // 1: BnB cube bounds read a half-precision copy of the bricked DT (rounded toward zero: lower bounds stay valid; each LOOKED-UP VALUE is low by < 2^-10 relative where its half is normal, i.e. from 2^-14 up to 65504 -- below, by < 2^-24 absolute; above,
	                              // it is 65504 -- and a bound's own deviation is larger: the radius subtracted from the value, v - rho, amplifies it); ICP, the DT re-score and trimmed bounds keep the fp32 grid.  No effect with
	                              // dt_layout = 0: the copy is made of the bricked grid only, a linear-layout engine keeps fp32 bounds.  Not bit-parity: opt-in
	int icp_nn_cache = 0;         // 1: an ICP pass skips (exactly) the tree walk of every query whose cached neighbour is provably still the nearest (measured slower on real trajectories, EXPERIMENTS 3.6: opt-in);
	                              // 2: the same, switched on inside a run only once the error falls by < 2 % per 16 iterations (the tail; measured +0..3 %, EXPERIMENTS R4.11: opt-in);
	                              // 0: every query walks every pass; bit-identical states in every mode
	int flow = 0;                 // opt-in; L > 0: continuous flow over the device queues -- rotation children are harvested one by one and the next batch of parents is admitted when at most this many inner searches still run; 0: lock-step batches
	int adaptive_k = 1;           // 1: when few inner searches still run, each may expand up to 512 nodes per round instead of trans_batch
	int queue_cap = 0;            // test hook: nodes a device queue may hold before the batch falls back to the host queues (0 = the full slab)
	int device_queues = 1;        // 1: inner-BnB queues live on the device, a round is two launches and no host work (bnbqueue.hip); 0: host queues (always used when trans_batch == 1 = the reference visit order)
	int icp_point_seed = 1;       // 1: the ICP neighbour search starts every walk from a real candidate read from a per-voxel nearest-target-point table
	                              // (built once with the k-d tree: the EDT passes carrying their arg-min; V^3 x 4 bytes); 0: from the distance-transform bound
	int ub_tiebreak = 0;          // opt-in, widened search only: rotation cubes with EQUAL lower bounds and equal width are expanded in the order of the smallest
	                              // upper bound their own inner search saw -- the reference leaves that order to its heap; 0: as the reference.  Measured (round 3,
	                              // DESIGN 4): ties are rare beyond level 2, no registration got faster -- default off
	float ub_share = 0.f;         // opt-in, widened search: on top of a batch's parents by smallest lower bound, this fraction more are drawn by the smallest upper
	                              // bound seen inside them (needs ub_tiebreak = 1 for the key).  Measured slower everywhere: default 0
	int sort_items = 1;           // rounds of >= 2 048 expansions walk their (expansion, chunk) items in the order of where their gathers land (device.hip, launch_queue_sort)
	int bounds_order = 2;         // tuning only.  Cube batches handed in on the device (eval_bounds_dev, lean bricked grid): 0 the groups are walked as they came; 1 a device pre-pass
	                              // orders them by run of equal rotation and Morton cell of the parent cube's centre (device.hip, bounds_order_kernel); 2 and two
	                              // neighbours of that order are evaluated together (lean_points_pair).  Same bits in every form
	int bounds_order_min_groups = 1024;   // tuning only: batches of fewer expansions keep the plain launch (the pre-pass is a launch of its own)
	int bounds_order_max_runs = 16;       // tuning only: batches with more runs of equal rotation (unrelated cubes) are walked as they came; at most 64
	float bounds_order_cell = 4.f;        // tuning only: smallest Morton cell of the order, in DT voxels
	int bounds_order_reprobe = 64;        // tuning only: after the pre-pass left a batch alone, batches of the same size skip the pre-pass (the parent's launch) and every
	                                      // this-many-th of them runs it again; 0: every batch runs it
	int bounds_balance = 1;               // the pair launch's 8-chunk shape: 1 a block label takes an equal share of the chunks' COST (distinct DT lines per wavefront,
	                                      // counted once per source cloud; device.hpp bounds_cuts), 0 one chunk each.  Same bits either way
	float bounds_balance_a = 0.f;         // tuning only: the weight of a wavefront against one DT line in that cost; <= 0: kBoundsBalanceA
	int bounds_dedup = 1;                 // the pair launch over several point chunks: 1 an expansion a run lists more than once (all eight records equal as raw bits) is
	                                      // evaluated once and its copies take the owner's sums (device.hip bounds_order_kernel, BoundsOrder::alias); 0 every listing is
	                                      // evaluated.  Same bits either way
	int twin_fusion = 1;         // the same translation node listed by both searches of a rotation child in a round is gathered once (device.hip lean_points<.., 2>)
	int lds_tiles = 2;            // LDS-staged DT tiles for inner searches whose selected nodes lie within a few voxels of each other (deep rounds): 0 off, 1 the
	                              // tile evaluation is launched every round, 2 only while the previous rounds had searches that qualify (default)
	float tile_spread_vox = 10.f; // ... "a few": largest extent of a search's selected translations, in DT voxels (measured: the tile kernel is 1.7x the gathering one at 3 voxels, 1.3x at 5, even at 10)
	int stale_widen = 1;          // adaptive_k: an inner search whose incumbent did not improve in its last round(s) is PROVING, not finding: every queued node whose lower
	                              // bound is more than SSEThresh below the incumbent has to be expanded whatever the order, so a wider round wastes nothing -- its width
	                              // doubles after one such round and again after three (lower-bound searches almost never improve; upper-bound searches until they settle)
	int stale_compact = 2048;     // a proving inner search whose queue holds at least this many nodes selects by Morton order of the cubes' corners instead of by lower
	                              // bound (spatially compact, depth-first-like: LDS-tile material, and the slab stops overflowing); 0: always by lower bound
	int tile_min = 8;             // ... and at least this many expansions (a lane group of the tile kernel is one expansion)
	int lanes = 0;                // n = 2..4 (always n) / 0 (auto: three, when the previous batch's rounds were throughput-bound; default) / 1 (never): a batch of at least
	                              // lane_min_searches inner searches is cut into lanes by rotation slot and the lanes run their lock-step rounds side by side on their own
	                              // streams (own lists, own control block): one lane's dependent launches drain beside the others' (run_inner_device)
	int lane_min_searches = 64;
	int stream_priority = 0;      // 1: the engine's stream gets the highest priority of the device (an ICP engine beside a bounds engine on one GPU: tools/overlap_probe.py)
	int icp_fused = 0;            // 1: one launch per ICP iteration (last workgroup finalizes); 0: pass + finalize launches (A/B).  Same per-point arithmetic; the sums are added in another order: states within float rounding of each other, equal to the bit only as observed, on the linear DT at 17 to 4 096 workgroups, and not above (tests/test_gpu_icp_forms.py)
	float trim_fraction = 0.f;    // GoICP::trimFraction (jly_goicp.h:116; the reference hard-wires 0, jly_goicp.cpp:55)
	// Search domain ([params.rotation] / [params.translation] of the reference's configs, test/skull_goicp.toml:22-41;
	// declared in src/common.h:157-169, never parsed there).  Unset = the CPU path's fixed domain
	// (jly_goicp.cpp:44-53): rotation cube [-pi,pi]^3, translation cube [-0.5,0.5]^3, no depth limit.
	int use_rot_range = 0, use_trans_range = 0;
	float rot_min[3] = {-180.f, -180.f, -180.f}, rot_max[3] = {180.f, 180.f, 180.f};   // degrees, angle-axis components
	float trans_min[3] = {-0.5f, -0.5f, -0.5f}, trans_max[3] = {0.5f, 0.5f, 0.5f};
	int rot_search_depth = 0, trans_search_depth = 0;   // 0 = unlimited; d: nodes of depth d are evaluated, not expanded
};

struct Counters {
	long long rot_pops = 0, trans_pops = 0, cubes = 0, inner_calls = 0, icp_runs = 0, icp_iters = 0;
	long long bounds_launches = 0;
	long long queue_fallbacks = 0;
	long long tile_expansions = 0;   // BnB expansions evaluated from LDS-staged DT tiles (8 cube bounds each; counted in `cubes` too)
	long long lane_batches = 0;      // batches of inner searches cut into two or more lanes
};

// what the viewer polls (fgoicp.hpp:34,67-69; goicp_kernel.cu:161-177)
struct Result {
	float optR[9], optT[3], curR[9], curT[3];
	float best_sse;
	int finished;
	Counters counters;
	double dt_build_ms, register_ms;
};

// corner + width node, ordered like jly_goicp.h:44-72 (smaller lb first, then the wider cube)
struct Node {
	float x, y, z, w, ub, lb;
	int l;
	float tie = 0.f;     // third key of the ROTATION queue in the widened search: the smallest upper bound seen inside the cube (0 = unused)
	friend bool operator<(const Node& a, const Node& b)
	{
		if (a.lb != b.lb) return a.lb > b.lb;      // smaller lower bound first, then the wider cube (jly_goicp.h:44-72)
		if (a.w != b.w) return a.w < b.w;
		return a.tie > b.tie;                      // equal in the reference's order (there the heap decides): the more promising cube first
	}
};

struct StepStatus {
	int finished;        // this rank has nothing left (queue empty, converged, or early exit)
	int early_exit;      // best_sse < sse_threshold (jly_goicp.cpp:527): every rank may stop
	float best_sse;
	float frontier_lb;   // min lb over this rank's queue (+inf when empty)
	long long rot_pops;
};

class Engine {
public:
	Engine(const Params& p, const float* target_xyz, size_t M, const float* source_xyz, size_t N);
	~Engine();
	Engine(const Engine&) = delete;

	// ---- operators (all synchronous) ----
	// Registration::compute_sse_error(RotNode&, vector<TransNode>&, fix_rot, StreamPool&) with the CPU
	// path's semantics: cubes = B x {centre xyz, child width}; level < 0 => no rotation radius.
	void eval_bounds(const float R[9], const float* cubes4, size_t B, int level, float* ub, float* lb);
	void eval_bounds_batch(const float* rots9, size_t K, const CubeRec* cubes, size_t B, float* ub, float* lb);
	void eval_bounds_dev(const Rot9* d_rots, const CubeRec* d_cubes, int B, float* d_ub, float* d_lb, hipStream_t s, const ParentRec* d_parents = nullptr);
	void reduce_min_dev(const float* d_v, int n, float* d_min, int* d_idx, hipStream_t s);
	float time_bounds_dev(const Rot9* d_rots, const CubeRec* d_cubes, int B, float* d_ub, float* d_lb, int iters, int grouped_nrots = 0);
	void eval_bounds_dev_grouped(const Rot9* d_rots, int nrots, const CubeRec* d_cubes, int B, float* d_ub, float* d_lb, hipStream_t s);
	float eval_sse(const float R[9], const float t[3]);
	float inner_bnb(const float R[9], int level, float incumbent, float best_node[4], Counters* c);
	float icp_run(float R[9], float t[3], int max_iter, float err_diff, int* iters);
	// goicp_icp_run_batch: K independent icp_run loops, one start pose each (R: K x 9, t: K x 3 in/out; err, iters: K, may be null), in one
	// device loop over the active poses; pose k ends bit for bit as icp_run from R + 9k, t + 3k.  The single-pose ICP state, the icp_step
	// pose, the poll snapshot and the neighbour cache are left alone
	void icp_run_batch(size_t K, float* R, float* t, int max_iter, float err_diff, float* err, int32_t* iters);
	// goicp_icp_run_collective: icp_run with the pass's workgroups split over the ranks of `comm` and the integer sums added up over
	// them -- every rank ends with the world-1 state, bit for bit.  Returns a goicp_status (collective: every rank returns together)
	int icp_run_collective(const goicp_comm_ops* comm, float R[9], float t[3], int max_iter, float err_diff, float* err, int* iters);
	const IcpShardStats& icp_shard_stats() const { return icp_shard_; }
	// goicp_register_sharded_collective_icp: while a communicator is set, the registration's refinements are collective -- the initial
	// ICP inside register_begin runs collectively, and an improved upper bound is adopted UNREFINED (the protocol refines the
	// global winner on every rank after the exchange, refine_collective)
	void set_collective_icp(const goicp_comm_ops* comm) { icp_comm_ = comm; unrefined_ = false; }
	bool pose_unrefined() const { return unrefined_; }
	// collective ICP from R|t, then the DT re-score (replicated); the current best pose counts as refined from here on
	float refine_collective(float R[9], float t[3]);
	float time_icp_pass(const float R[9], const float t[3], int iters, bool cached = false);   // cached: every query hits the neighbour cache (steady state); else every query walks
	void nn_query(const float* q_xyz, size_t n, int32_t* idx, float* d2);
	// goicp_icp_options: the metric of every ICP this engine runs (0 point-to-point, 1 point-to-plane) and the neighbours per target
	// normal; metric 1 builds the normals (once per normal_k).  Refused while a registration runs and together with trimming
	void set_icp_options(int metric, int normal_k);
	int icp_metric() const { return icp_metric_; }
	// goicp_set_icp_symmetric: a modifier of metric 1 -- the symmetric point-to-plane objective over the normals of both clouds (include/goicp_mi355.h).
	// Stored and inert under metric 0.  source_normal_k: the neighbours per estimated source normal.  Refused: source_normal_k outside 3..32 or
	// above the source's size, enabled together with trimming or with a gate whose min_inliers is below 6, while a registration runs
	void set_icp_symmetric(int enabled, int source_normal_k);
	bool icp_symmetric() const { return icp_symmetric_; }
	int source_normal_k() const { return source_normal_k_; }
	bool user_source_normals() const { return src_normals_user_; }
	void check_symmetric_query(const char* fn) const;            // what every entry point of the feature refuses: a running registration
	// goicp_set_icp_generalized: the other modifier of metric 1 -- generalized (plane-to-plane) ICP, a 3 x 3 weight per correspondence from the
	// normals of both clouds (include/goicp_mi355.h).  Stored and inert under metric 0; it shares source_normal_k and the source normals with
	// the symmetric flag, and the two refuse each other.  Refused beyond that: epsilon outside [1e-4, 1], and what set_icp_symmetric refuses
	void set_icp_generalized(int enabled, float epsilon, int source_normal_k);
	bool icp_generalized() const { return icp_generalized_; }
	float gicp_epsilon() const { return gicp_eps_; }
	void source_normals(float* normals_xyz);                     // N x 3, original source order (built on first use)
	// the caller's own normals (original source order; each exactly zero or of length within 1e-3 of 1), in the place of the estimated ones
	// until the next source swap
	void set_source_normals(const float* normals_xyz, size_t n);
	// goicp_icp_gate: a maximum correspondence distance for every ICP this engine runs (0 = off).  A correspondence is an inlier iff the walk's
	// d^2 <= max_corr_dist^2; sums, update and stop rule run over the inliers (device.hip gate_step).  min_inliers 0 = the metric's floor (3 / 6).
	// Refused: a negative or non-finite distance, min_inliers below the floor, a gate with trimming, with dt_layout 0 or with icp_fused, while
	// a registration runs
	void set_icp_gate(float max_corr_dist, int min_inliers, int capped_walk);
	bool icp_gated() const { return gate_dist_ > 0.f; }
	// goicp_icp_robust: an M-estimator for every ICP this engine runs (kernel 0 = off; 1 Huber, 2 Cauchy, 3 Geman-McClure, 4 Tukey; scale c > 0).
	// Every term of the update is multiplied by the weight w of the correspondence's residual, W = sum w takes n's place, and the stop rule
	// reads the robust cost C = sum rho (device.hip robust_terms / robust_step).  Refused: a kernel outside 0..4, a scale that is not finite
	// and > 0, a kernel with trimming, with a gate, with dt_layout 0 or with icp_fused, while a registration runs
	void set_icp_robust(int kernel, float scale);
	// goicp_set_search_truncation: the objective of the SEARCH (0 = off, the plain L2 objective).  g > 0: every term of every cube bound and
	// of every pose score is clamped at g -- E_g(R, t) = sum min(DT(R p + t), g)^2, upper-bound term min(m, g)^2, lower-bound term
	// min(max(m - delta, 0), g)^2 (device.hip trunc_clamp).  g rides in DtDesc::trunc of both grids, so every launch that takes bounds_dt() or
	// dt_ -- eval_bounds_dev(_grouped), the device-queue and tile rounds, run_inner_host, inner_bnb, the debug entries, eval_sse and with it the
	// re-scores of icp_from and register_begin -- evaluates the truncated form; SSEThresh, pruning, early exit and adopt-on-improvement are
	// untouched.  Refused: a negative or non-finite distance, truncation with trimming, while a registration runs
	void set_search_truncation(float g);
	float search_truncation() const { return dt_.trunc; }
	bool icp_robust() const { return robust_kernel_ != 0; }
	// C and W of the last pass of the last icp_run (K = 1) or icp_run_batch (its K); any other K is refused; either output may be null
	void icp_robust_stats(size_t K, float* cost, float* weight_sum) const;
	// inlier counts of the last icp_run (K = 1) or icp_run_batch (its K); any other K is refused
	void icp_inliers(size_t K, int32_t* out) const;
	// goicp_eval_correspondences: per source point (original order) the neighbour's index (-1 beyond the gate) and d^2 at R|t, the inlier count
	// and the inliers' sum of d^2 (double sum in source order, rounded once); max_corr_dist 0 = no gate; any output may be null
	void eval_correspondences(const float R[9], const float t[3], float max_corr_dist, int32_t* index, float* dist_sq, int32_t* inliers, float* sse);
	// goicp_pose_information(_batch): the Gauss-Newton normal matrix and gradient of either metric at K given poses under the handle's weights
	// (plain, gate, robust kernel), about the caller's pivot or the transformed source centroid, and the fp64 finishing step per pose
	// (DESIGN 15).  batch: the blockIdx.y form (slot k is the single call at pose k bit for bit).  Touches no ICP or search state.
	// Refused: trimming, dt_layout 0, icp_fused, a metric outside {-1, 0, 1}, non-finite R / t / pivot, a pivot that would overflow the
	// fixed-point sums, rank_tol outside [0, 1), K outside 1..1024, while a registration runs
	void pose_information(size_t K, const float* R, const float* t, const goicp_pose_info_options* opt, goicp_pose_info* out, bool batch);
	void result_information(const goicp_pose_info_options* opt, goicp_pose_info* out);   // at optR | optT of the last finished registration
	static constexpr double kPoseInfoRankTol = kIcpRankTol;
	void knn_query(const float* q_xyz, size_t n, int k, int32_t* idx, float* d2);
	double normal_build_ms() const { return normal_build_ms_; }   // exact, ascending (d2, index), n x k
	double source_normal_build_ms() const { return source_normal_build_ms_; }
	void target_normals(float* normals_xyz);                                         // M x 3, original target order (built on first use)
	void icp_step();   // one ICP iteration on the engine's current pose (ICP::kdTreeGPUStep)
	// measured ceiling of the gather path (4-byte loads into the resident DT): lookups/s; mode 0 coalesced, 1 divergent
	double probe_gather(int mode, size_t window_bytes);
	long long debug_cache_hits(const float R[9], const float t[3]);   // queries of a repeated pass that skipped the tree walk (-1: cache off)
	// test: the trimmed ICP's selection of the num smallest of d2[0..n) on the device, as inclusion flags (kernel 0 = the iteration's
	// choice by size, 1 = register kernel, n <= 32 768, 2 = streaming kernel)
	void debug_select(const float* d2, size_t n, int num, int kernel, unsigned char* include);
	// test: the n (<= 128) given translation nodes (parents4: corner xyz + width) expanded by ONE round of the device-resident queues -- an
	// upper-bound search (coeff 0) and a lower-bound search (rotation level `level`) of the same rotation, twins of each other, both listing
	// all n nodes: the round the outer search's lock-step batches run (selection by bnb_queue_kernel, evaluation by bounds_queue_kernel with
	// twin fusion when the engine has it on).  out[pass][8 n]: the children's bounds of pass 0 (upper-bound search) and pass 1
	// (lower-bound search), in the order of parents4.  info[0] = point chunks the evaluation split the cloud into, info[1] = 1 when the
	// twin lists were in use.
	void debug_bounds_order(int info[3]);   // test: form of the last eval_bounds_dev launch, and what its pre-pass decided (device.hip BoundsOrder::ctl)
	void debug_bounds_twins(int info[2]);   // test: items of that launch evaluated in twin form and in identical form (BoundsOrder::ctl[2], [3])
	void debug_bounds_copies(int info[1]);  // test: groups of that launch not evaluated, being copies of another group of their run (BoundsOrder::ctl[kBoundsCopies])
	// test: the cuts of that launch and the source's chunk cost: info[0..8] cut, [9..16] lines, [17..24] waves, [25] 1 = the cuts followed the cost
	// (pair form, 8 chunks, bounds_balance); a launch without the 8-chunk pair form reports the equal split of its items
	void debug_bounds_balance(int info[26]);
	// diagnostic build (GOICP_BOUNDS_XCD_STAMPS) only: the stamps of the pair launches since the last call, which clears them
	// (device.hpp kXcdStampRows x kXcdStampCols); false in the shipped library
	bool debug_bounds_xcd_spans(unsigned long long* out);
	void debug_queue_expand(const float R[9], int level, const float* parents4, int n, float* ub0, float* lb0, float* ub1, float* lb1, int info[2]);
	// test: the same round with the TILE list on (tile_min 1, no spread limit): both searches list their nodes there and nothing in the direct
	// list; the upper-bound search queues only the first n_ub nodes (out arrays: 8 n_ub and 8 n floats).  info = {tile chunks the device chose,
	// tile segments, workgroups of the tile launch, twin lists in use}.  The tile buffers are filled with NaN before the round: a row the
	// evaluation never wrote cannot pass for one it did.  dg (may be null): the queue kernel is launched once more (K = 1) and
	// digests the round from the tile buffers -- what it pushed, what it listed next and the searches' incumbents come back in *dg.
	struct QueueDigest {
		float* nodes;      // [2][8 n][6]: the queue of search s after the digest and the next selection (corner, width, ub, lb per node)
		int* counts;       // [2][2]: nodes in that queue, nodes the selection took out of it
		float* listed;     // [2][4]: the node taken (corner, width), when one was
		float* search;     // [2][8]: best, min_ub, improved, bx, by, bz, bw, done
	};
	void debug_queue_expand_tiles(const float R[9], int level, const float* parents4, int n, int n_ub, float* ub0, float* lb0, float* ub1, float* lb1, int info[4],
	                              const QueueDigest* dg);
	// test: launch_bnb_queue once on caller-given searches, queues, previous list and children's bounds (goicp_debug_queue_round, goicp_mi355.h),
	// in device buffers of the call's own: no bound evaluation, no cloud, no distance transform; the engine's lanes, lists and counters are not
	// touched.  std::invalid_argument before any launch for arguments outside the documented ranges
	void debug_queue_round(const goicp_queue_round& rp, goicp_queue_search* searches, float* nodes, const void* prev_parents, const float* prev_ub,
	                       const float* prev_lb, const float* prev_scratch, int32_t ctl[6], void* listed, int32_t* parent_search);
	// measurement / test: the 8 children of nseg x n expansions (segment i: rotation i, parents4[(i*n + e)*4 ..] = corner xyz + width) through
	// the LDS-tile kernel and through the direct kernel; out arrays hold 8*nseg*n floats each; ms[0] tile, ms[1] direct (per launch)
	void debug_bounds_tile(const float* rots9, const float* parents4, int nseg, int n, int level, int chunks, float* ub_tile, float* lb_tile,
	                       float* ub_direct, float* lb_direct, float ms[2], unsigned stats[2]);

	// ---- registration ----
	void run();                                  // FastGoICP::run / GoICP::Register
	void cancel() { cancel_.store(true); }
	Result poll();
	// called on the registering thread after every published snapshot (the reference's worker writes
	// FastGoICP::optR/optT/curR/curT itself, fgoicp.cpp:68-69,85-86)
	void set_progress_callback(std::function<void(const Result&)> cb) { progress_cb_ = std::move(cb); }
	// stepped form for multi-GPU sharding
	void set_shard(int rank, int world) { rank_ = rank; world_ = world; }
	void register_begin();
	StepStatus register_step(int max_rot_pops);
	void offer_global_best(float sse, const float R[9], const float t[3]);   // result of the min all-reduce
	void register_end();
	// rebalancing between ranks (shard.cpp): cubes still worth expanding / give every second one away / take some
	int queue_size() const { return (early_exit_ || converged_) ? 0 : (int)queue_.size(); }
	int donate(int max_nodes, float* nodes7);
	void receive(const float* nodes7, int n);

	// ---- inspection ----
	const DtDesc& dt() const { return dt_; }
	void dt_download(float* grid_linear);        // V^3, [z][y][x]
	size_t n_source() const { return N_; }
	size_t n_target() const { return M_; }
	const float* target_xyz() const { return h_target_.data(); }
	float sse_threshold() const { return sse_thresh_; }
	int device() const { return dev_; }
	int inliers() const { return inliers_; }
	float rot_coeff(int level) const;
	hipStream_t stream() const { return stream_; }
	const float4* d_source() const { return d_src_.get(); }
	void source_transformed(const float R[9], const float t[3], float* out_xyz);  // original order
	// goicp_set_source: a new source cloud under the same target -- everything derived from the target is kept (distance transform, k-d
	// hierarchy, nearest-point table, normals, streams, queues, warm-ups), the params and the per-handle options persist, the search / ICP
	// state is the one of a fresh engine.  The order is computed on the device (kdbuild.hip).  Refused while a registration runs.  fn: the C
	// entry point the caller used, which the refusals, the trace range and the verbose line name
	void set_source(const float* source_xyz, size_t N, const char* fn = "goicp_set_source");
	// goicp_set_source_voxel / _filtered / _pipeline / _clustered: one chain, of which each entry point can switch on its share of the stages
	// voxel grid -> statistical filter -> radius filter -> plane removal -> cluster selection (a stage whose size is 0 is off; with none on it is
	// set_source).  The raw cloud goes up once, each stage reads the one before it on the device, only the final cloud and the permutation
	// come back; afterwards the engine is the one set_source(the composition of the host functions) leaves.  What the arguments and the raw
	// cloud show is refused before any device work (the first stage that runs checks the raw cloud on the host and takes its frame from
	// it); what only an intermediate cloud shows (k above its size, the 2^16 rule of a later grid, a stage that keeps no point) when that
	// cloud exists, still before load_source: a refused call leaves the engine as it was
	struct SourceStages {
		float voxel = 0.f;
		int32_t stat_neighbors = 0;
		float stat_std_ratio = 0.f;
		float radius = 0.f;
		int32_t min_neighbors = 0;
		float cluster_radius = 0.f;
		int32_t cluster_min_neighbors = 0, cluster_min_size = 0, cluster_max_clusters = 0;
		// plane removal (between the radius and the cluster stage): plane_distance == 0 is no stage; the fields of goicp_plane_select
		float plane_distance = 0.f;
		int32_t plane_iterations = 0, plane_refine = 0, plane_max = 0, plane_min_inliers = 0;
		uint64_t plane_seed = 0;
	};
	void set_source_staged(const char* fn, const float* xyz, size_t n, const SourceStages& st, size_t* n_kept);
	// goicp_debug_source_order (test): the device ordering alone, of any cloud
	void debug_source_order(const float* xyz, size_t n, int mode, int32_t* perm);
	double last_source_order_ms() const { return source_order_ms_; }   // the device ordering of the last set_source (HIP events)
	// goicp_voxel_downsample: the voxel-grid reduction on the device (kdbuild.hip launch_voxel_downsample); the engine lends its device and
	// stream and nothing else: no member is written.  Refused while a registration runs
	void voxel_downsample(const float* xyz, size_t n, float voxel, float* out_xyz, int32_t* out_count, size_t* m);
	// goicp_radius_outlier_removal: the radius filter on the device (kdbuild.hip launch_radius_outlier_removal); as voxel_downsample, the
	// engine lends its device and stream and nothing else
	void radius_outlier_removal(const float* xyz, size_t n, float radius, int32_t min_neighbors, float* out_xyz, int32_t* out_index, int32_t* out_count,
	                            size_t* m);
	// goicp_statistical_outlier_removal: the statistical filter on the device (kdbuild.hip launch_stat_outlier_removal); as voxel_downsample,
	// the engine lends its device and stream and nothing else
	void statistical_outlier_removal(const float* xyz, size_t n, int32_t neighbors, float std_ratio, float* out_xyz, int32_t* out_index,
	                                 float* out_mean_dist, double* threshold, size_t* m);
	// goicp_knn_self / goicp_estimate_normals: the exact self k-NN and the normals of any cloud on the device (kdbuild.hip launch_self_knn /
	// launch_estimate_normals); as statistical_outlier_removal, the engine lends its device and stream and nothing else
	void knn_self(const float* xyz, size_t n, int32_t k, int32_t* out_index, float* out_dist_sq);
	void estimate_normals(const float* xyz, size_t n, int32_t k, const float* vp, float* out_normals, float* out_variation, int32_t* out_index);
	// goicp_fpfh / goicp_match_features: the descriptors of any cloud and the nearest-descriptor search on the device (kdbuild.hip launch_fpfh /
	// launch_match_features); the engine lends its device and stream and nothing else
	void fpfh(const float* xyz, const float* normals, size_t n, int32_t k, float* out_fpfh, uint8_t* out_spfh_counts);
	void match_features(const float* q, size_t nq, const float* t, size_t nt, int32_t* out_index, float* out_d2, float* out_d2_second, uint8_t* out_mutual);
	// goicp_cluster / goicp_cluster_filter: Euclidean / DBSCAN clustering and the cluster selection on the device (kdbuild.hip launch_cluster /
	// launch_cluster_compact; the selection itself runs on the host over the c sizes); the engine lends its device and stream and nothing else
	void cluster(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t* out_label, int32_t* out_sizes, size_t* n_clusters);
	void cluster_filter(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t min_size, int32_t max_clusters, float* out_xyz,
	                    int32_t* out_index, int32_t* out_label, size_t* m);
	// goicp_segment_plane / goicp_plane_filter: RANSAC plane segmentation on the device (kdbuild.hip launch_segment_plane; the refit's finish
	// runs on the host over 16 integer words); the engine lends its device and stream and nothing else.  s: the checked selection
	void segment_plane(const float* xyz, size_t n, const PlaneSelect& s, int32_t* out_label, PlaneRecord* out_planes, size_t* n_planes);
	void plane_filter(const float* xyz, size_t n, const PlaneSelect& s, float* out_xyz, int32_t* out_index, PlaneRecord* out_planes, size_t* n_planes, size_t* m);
	// goicp_ransac_pose: RANSAC pose estimation from correspondences on the device (kdbuild.hip launch_ransac_pose; the refit's finish runs on
	// the host over 25 integer words per pose); the engine lends its device and stream and nothing else.  s: the checked selection
	void ransac_pose(const float* src, size_t n_s, const float* tgt, size_t n_t, const int32_t* corr, size_t M, const RansacPoseSelect& s,
	                 RansacPoseRecord* out_poses, size_t* n_poses, uint8_t* out_inlier);

private:
	Engine(const Params& p, size_t M, size_t N);     // the members' defaults; the public constructor delegates to it and runs init
	struct InnerSearch;
	void init(const float* target_xyz, size_t M, const float* source_xyz, size_t N);
	static void check_source(const float* source_xyz, size_t N);
	// the source stage of init and all of set_source's device work: order (host, or device when device_order) -> gather with |p| ->
	// centroid -> upload -> the N-sized buffers (grow-only)
	// d_xyz_ready: the same cloud already on the device (3 N floats; set_source_staged), which the device order then reads instead of an upload
	void load_source(const float* source_xyz, size_t N, bool device_order, const float* d_xyz_ready = nullptr);
	void finish_source_swap();                       // set_source / set_source_staged after load_source: the search and ICP state of a fresh engine
	void sync_lane_streams();                        // a swap waits for what the lanes still have in flight before it touches the source buffers
	double source_order_ms_ = 0;
	void ensure_batch(size_t B, size_t K);
	void ensure_stage(size_t B);
	const BoundsOrder* ensure_bounds_order(int B, hipStream_t s);   // the order / pair buffers for a launch of B cube bounds (nullptr: the plain launch); grows like the scratch
	Buf<unsigned> d_border_;
	PinnedBuf<long long> h_border_note_;  // what the last pre-pass found (BoundsOrder::host_note): read without a wait, a hint only -- every form gives the same bits
	int border_skipped_ = 0;
	int border_form_ = 0;                // the form of the last eval_bounds_dev launch, and the stream it went to (debug_bounds_order)
	hipStream_t border_stream_ = nullptr;
	BoundsOrder border_{};
	Buf<int> d_bcost_;                   // lines[8], waves[8] of the source's chunks and the plan of the cuts (BoundsOrder::cost); update_bounds_cost, on the engine's stream
	int border_chunks_ = 0, border_items_ = 0;   // chunks and groups-derived equal-split items of the last launch (debug_bounds_balance)
	void update_bounds_cost();
	void ensure_bounds_scratch(int B, hipStream_t s);   // d_scratch_ holds a launch of B cube bounds; growing waits for stream_ and s only
	void upload_rots(const std::vector<Rot9>& rots);    // the batch's rotation table -> d_rots_, on stream_
	void run_inner(std::vector<InnerSearch*>& searches, const std::vector<Rot9>& rots);
	void run_inner_host(std::vector<InnerSearch*>& searches, const std::vector<Rot9>& rots, bool fallback = false);
	bool run_inner_device(std::vector<InnerSearch*>& searches, const std::vector<Rot9>& rots);   // false: a round's lists overflowed, nothing was changed; redo_: searches whose own queue did
	std::vector<InnerSearch*> redo_;
	void process_parents(const std::vector<Node>& parents);
	struct Kid { Node node; float R[9]; float parent_lb; };                       // a rotation child and its Rodrigues matrix
	struct SearchOut {   // what an inner search returns (min_ub: smallest upper bound of any cube it evaluated)
		float best; bool improved; Node best_node; long long pops, cubes; float min_ub;
		static SearchOut of(const InnerSearch& s);   // from the host's record of a search
		static SearchOut of(const QSearch& q);       // from the device queues' record
	};
	InnerSearch fresh_search(int rot_slot, float coeff, float incumbent) const;   // a search about to start: the translation root queued (jly_goicp.cpp:50-53)
	// octant j of a cube: the same float expressions wherever a cube is split (jly_goicp.cpp:262-273, :427-441)
	static Node child_cube(const Node& parent, int j)
	{
		Node c{};
		c.w = parent.w / 2;
		c.x = parent.x + (j & 1) * c.w; c.y = parent.y + (j >> 1 & 1) * c.w; c.z = parent.z + (j >> 2 & 1) * c.w;
		return c;
	}
	// up to P rotation parents off the queue, by the stop rule of jly_goicp.cpp:416; may_converge: a first parent inside SSEThresh ends the search
	std::vector<Node> pop_parents(int P, int max_rot_pops, int& pops, bool may_converge);
	void make_kids(const std::vector<Node>& parents, std::vector<Kid>& kids);
	bool handle_ub(Kid& k, const SearchOut& s);
	void handle_lb(Kid& k, const SearchOut& s);
	// continuous flow of the outer search over the device-resident queues (engine.cpp)
	static constexpr int kFlowSearches = 2048;     // search slots (two per rotation child in flight)
	struct Flight { Kid kid; int rot_slot, s_ub, s_lb; float incumbent; bool handled; };
	bool flow_mode() const { return p_.device_queues && p_.wide_children && p_.trans_batch > 1 && p_.flow; }
	int flow_step(int max_rot_pops);
	void flow_reset();
	void flow_fallback();
	QParams queue_params() const;
	std::vector<Flight> flights_;
	std::vector<int> free_search_, free_rot_;
	int q_hi_ = 0, q_parity_ = 0, flow_active_ = 0;
	void adopt(float err, const float R[9], const float t[3]);
	float icp_from(float R[9], float t[3]);
	void publish(bool finished);
	void icp_state_init(const float R[9], const float t[3], float err_diff, int carry_means, int frozen);
	void icp_state_fill(IcpState& st, const float R[9], const float t[3], float err_diff, int carry_means, int frozen) const;   // host half of icp_state_init
	void icp_state_fetch();

	// HIP's current device is per host thread: every public entry point re-establishes the engine's device
	struct DeviceGuard {
		int prev = -1, want = -1;
		explicit DeviceGuard(int dev);
		~DeviceGuard();
	};
	// A cube is the half-open box [x, x+w)^3, a configured range the CLOSED box [lo, hi]: the cube is kept when the two
	// intersect.  So the high face of a range is inclusive -- a bound (or a fixed value, lo == hi) that coincides with a
	// split plane belongs to exactly one cube per level, the one that starts there -- and the low face of a cube that
	// merely ends at lo is not.  Same rule on the device (bnbqueue.hip in_box).
	bool in_box(const Node& c, const float lo[3], const float hi[3]) const { return cube_in_range(c.x, c.y, c.z, c.w, lo, hi); }
	void* scratch_bytes(size_t bytes);   // grow-only device scratch for the query / transform operators

	Params p_;
	int dev_ = 0;
	Node rot_root_{}, trans_root_{};
	bool rot_boxed_ = false, trans_boxed_ = false;
	float rot_lo_[3], rot_hi_[3], trans_lo_[3], trans_hi_[3];
	std::function<void(const Result&)> progress_cb_;
	size_t M_ = 0, N_ = 0;
	float sse_thresh_ = 0.f, icp_err_diff_ = 0.f;
	int inliers_ = 0;             // inlierNum = (int)(Nd * (1 - trimFraction)), jly_goicp.cpp:201
	int rank_ = 0, world_ = 1;

	// ---- what the engine owns on the device.  Members go in reverse order of declaration: the caller's device is restored after everything
	// else is gone (~Engine made the engine's device current), and the streams outlive the buffers and events used on them ----
	struct RestoreDevice { int prev = -1; ~RestoreDevice(); } restore_device_;
	static constexpr int kMaxLanes = 4;
	Stream stream_;
	Stream lane_own_[kMaxLanes];                            // [0] stays empty: lane 0 runs on stream_
	hipStream_t lane_stream_[kMaxLanes] = {};               // lane 0: stream_, lane 1: created with the engine, further lanes: on first use
	void make_lane_stream(int li);
	Event ev0_, ev1_;
	Event ev_fork_;                   // the other lanes of a batch start behind the engine's stream (run_inner_device)
	Buf<unsigned char> d_opscratch_;  // scratch_bytes
	PinnedBuf<QInit> h_qinit_; Buf<QInit> d_qinit_;
	Buf<float4> d_src_;               // N  (x,y,z,|p|), k-d order (Params::morton_sort); grow-only, as every N-sized buffer below
	std::vector<int32_t> src_perm_;   // sorted position -> original index
	std::vector<float> h_src_sorted_; // N*4
	std::vector<float> h_target_;     // M*3 (kept for viz.ply)
	float src_centroid_[3] = {0, 0, 0}, model_centroid_[3] = {0, 0, 0};
	DtDesc dt_{};
	Buf<float> d_dt_;
	DtDesc dt16_{};                   // Params::bounds_fp16: the same grid in half precision (layout 2)
	Buf<unsigned short> d_dt16_;
	size_t kd_slots_ = 0;                 // float4 slots behind KdDesc::pts
	Buf<int32_t> d_nn_ids_;               // nearest-target-point table of the ICP neighbour search (DtDesc::nn_ids)
	bool score_exact_ = false;        // set while eval_sse scores a pose: always the fp32 grid
	const DtDesc& bounds_dt() const { return (d_dt16_ && !score_exact_ && inliers_ >= (int)N_) ? dt16_ : dt_; }
	Buf<double> d_overshoot_;
	// k-d tree
	KdDesc kd_{};
	Buf<float> d_kd_boxes_[kMaxLevels]; Buf<float4> d_kd_pts_;
	// bounds staging
	size_t cap_cubes_ = 0, cap_rots_ = 0;   // what the six cube buffers / the two rotation buffers hold (0 while one of them is missing)
	Buf<CubeRec> d_cubes_; PinnedBuf<CubeRec> h_cubes_;
	Buf<Rot9> d_rots_; PinnedBuf<Rot9> h_rots_;
	Buf<float> d_ub_, d_lb_; PinnedBuf<float> h_ub_, h_lb_;
	Buf<float> d_scratch_;
	struct Stage {   // staging of a round of the host-queue inner BnB (run_inner_host)
		Buf<ParentRec> d_parents; PinnedBuf<ParentRec> h_parents;   // one record per expansion; the kernels derive the 8 children
		Buf<float> d_ub; PinnedBuf<float> h_ub;   // ub[B] followed by lb[B]
		size_t cap = 0, B = 0; Event ev;          // cap: cube bounds the four buffers hold
	} stage_;
	// device-resident inner-BnB queues (bnbqueue.hip).  A LANE is one self-contained set of them -- search slots, node slabs, the
	// round's two expansion lists with their bounds and partial sums, the sort buffers, the control block with its pinned snapshots --
	// driven on its own stream.  Lane 0 always exists; lane 1 is created for batches cut in two (Params::lanes, run_inner_device)
	struct QLane {
		hipStream_t stream = nullptr;                       // lane_stream_[li]: not the lane's to destroy
		size_t cap = 0;                                     // search slots
		Buf<QSearch> d_search; PinnedBuf<QSearch> h_search;
		Buf<QNode> d_nodes;
		Buf<ParentRec> d_parents[2];
		QSort sort{};                                       // footprint-ordered items of large rounds (device.hip); order == nullptr: off
		Buf<unsigned> sort_keys, sort_order, sort_hist; Buf<float4> sort_cen;   // ... what `sort` points into
		int list_cap = 0;                                   // expansions the round's lists (parents, bounds, partial sums) hold
		int seg_cap = 0;                                    // segments the tile list holds (list_cap / 64 + search slots)
		Buf<int> d_psearch[2];                              // per listed expansion: the search that listed it (twin test of the bound evaluation)
		Buf<float> d_ub, d_lb, d_scratch;
		Buf<QCtl> d_ctl; PinnedBuf<QCtl> h_ctl;             // h_ctl: the pinned snapshot of the last read-back
		Event ev_ctl;                                       // recorded behind that read-back
		QTile tile{};                                       // the tile list's buffers (null when lds_tiles == 0 or the DT is not bricked fp32)
		Buf<ParentRec> tile_parents[2]; Buf<TileSeg> tile_segs[2]; Buf<float> tile_ub, tile_lb, tile_scratch;   // ... what `tile` points into
		int tile_hint_seen = 0;                             // QCtl::tile_hint at the last read-back
		void drop_sort();                                   // the sort's / the tile list's buffers go and the descriptor reads "off"
		void drop_tile();
	} ql_[kMaxLanes];
	void lane_source_buffers(QLane& L);   // what a lane derives from the source: the sorted-round setup, the scratch sized by it, the tile list
	void ensure_lane(int li, size_t nsearch);
	// one round of a lane (engine.cpp queue_round).  tiles / twins: the tile list / the twin lists are in use; deep: the 64-VGPR build of the queue kernel
	// (the launcher's default); sorted: footprint-ordered items; read_ctl: QCtl is read back behind the round's selection (ev_ctl); count: the round counters move
	struct RoundOpts { bool tiles = false, twins = false, deep = true, sorted = false, read_ctl = false, count = true; };
	void queue_round(QLane& L, int nsearch, const QParams& qp, int parity, int max_groups, const RoundOpts& o);
	double last_round_work_ = 0;                            // point-expansions (expansions x source points) of the previous batch's mean round
	static constexpr double kLaneMinWork = 64e6;            // the auto mode's bar on last_round_work_ (run_inner_device)
	static constexpr int kAutoLanes = 3;                    // lanes the auto mode cuts a batch into (measured 2 / 3 / 4 at the end of round 4: bunny mse 3e-5
	                                                        // 5.06 / 5.02 / 5.48 s, synthetic 40 k mse 3e-5 621 / 621 / 681 ms, 3 k points mse 3e-5 1 033 / 1 016 / 1 100 ms, bunny mse 1e-4 259 / 261 / 268 ms)
	int lanes_ = 0, lane_min_searches_ = 64;                // Params::lanes / lane_min_searches
	bool tiles_usable() const;
	// shared by debug_queue_expand and debug_queue_expand_tiles (engine.cpp)
	bool debug_queue_setup(QLane& L, const float R[9], int level, const float* parents4, const int cnt[2]);
	void debug_queue_fetch(QLane& L);
	void debug_queue_gather(QLane& L, const ParentRec* d_list, int total, int chunks, const float* d_scratch, const float* d_ub, const float* d_lb, bool exact_sum,
	                        const float* parents4, const int cnt[2], float* const out[4]);
	long long sel_hist_[4][4] = {};       // verbose: QCtl::sel_hist summed over the registration
	bool tile_sticky_ = false;            // lds_tiles == 2: the previous batch evaluated expansions from tiles -> this batch launches the tile list in every round
	static constexpr double kTileStickyShare = 0.5;   // ... when at least this share of the previous batch's cube bounds came from tiles
	long long tile_rounds_ = 0;           // rounds whose tile evaluation was launched
	long long queue_rounds_ = 0, queue_fallbacks_ = 0;
	// icp staging
	Buf<float> d_icp_partials_; Buf<IcpState> d_icp_state_; PinnedBuf<IcpState> h_icp_state_;
	Buf<unsigned long long> d_icp_acc_;         // fixed-point sums of the small-cloud ICP pass (kIcpAccReplicas x 16, zero between iterations)
	float src_radius_ = 0.f, target_abs_max_ = 0.f;   // extents that bound the pass's terms (IcpState::acc_scale)
	Buf<float4> d_nn_cache_;           // per source point: {q_ref, sqrt(best2_ref)}, {neighbour, index} (exact walk-skipping, device.hip)
	bool icp_cache_active_ = false;    // icp_nn_cache = 2: switched on inside a run once the error's decrease per chunk falls under kIcpCacheRel (the tail of a run)
	static constexpr float kIcpCacheRel = 0.02f;
	bool count_hits_ = false;
	Buf<int> d_icp_ticket_;            // arrival ticket of the fused ICP iteration (zero between launches)
	Buf<float> d_nn_d2_; Buf<int> d_nn_slot_; Buf<unsigned char> d_include_;   // trimmed ICP only
	void icp_launch_one();
	int icp_mode() const { return icp_robust() ? kIcpModeRobust : icp_gated() ? kIcpModeGate : kIcpModePlain; }   // launch_icp_iteration_opt's
	void icp_last_stats(const IcpState* fin, size_t K);
	// the collective ICP loop: the exported totals + converged flag + loop state read back per iteration, the summed totals uploaded
	Buf<long long> d_icp_x_; PinnedBuf<long long> h_icp_x_;
	IcpShardStats icp_shard_;
	// point-to-plane ICP (opt-in): the metric, the normals (one float4 per target point, original order: the pass gathers by the neighbour's index)
	int icp_metric_ = 0, normal_k_ = 16, normals_k_ = 0;   // normals_k_: the normal_k the normals were built with (0: none yet)
	Buf<float4> d_normals_;
	double normal_build_ms_ = 0;
	// the fixed-point accumulators of every single-pose opt-in iteration (point-to-plane, gate, kernel; one runs at a time):
	// kIcpAccReplicas x kIcpPlaneStride, zero between iterations
	Buf<unsigned long long> d_icp_acc_opt_;
	void ensure_icp_acc_opt();
	// distance-gated ICP (opt-in): the gate
	float gate_dist_ = 0.f; int gate_min_inliers_ = 0, gate_capped_ = 1;
	std::vector<int32_t> last_inliers_;                    // icp_inliers: the last run's counts
	int gate_floor() const { return icp_metric_ == 1 ? 6 : 3; }
	// robust-kernel ICP (opt-in): kernel and scale (a gate and a kernel exclude each other)
	int32_t robust_kernel_ = 0; float robust_scale_ = 0.f;
	std::vector<float> last_robust_cost_, last_robust_w_;  // icp_robust_stats: the last run's C and W
	std::atomic<int> registering_{0};                      // register_begin .. register_end: the options may not change
	// goicp_icp_run_batch (allocated on first use, grown on demand): cap pose slots of loop state and accumulators (kIcpBatchAccWords each,
	// zero between iterations), the pinned mirror of the states (one upload slot + two fetch slots), two active lists (device + pinned)
	Buf<IcpState> d_batch_states_; PinnedBuf<IcpState> h_batch_states_;
	Buf<unsigned long long> d_batch_acc_;
	Buf<int> d_batch_active_; PinnedBuf<int> h_batch_active_;
	size_t batch_cap_ = 0;             // pose slots all five hold (0 while one of them is missing)
	void ensure_icp_batch(size_t K);
	void ensure_normals(int k);
	// symmetric point-to-plane ICP (opt-in): the flag, the source normals (one float4 per source point, parallel to d_src_: the pass loads by query)
	bool icp_symmetric_ = false, src_normals_user_ = false;
	int source_normal_k_ = 16, src_normals_k_ = 0;        // src_normals_k_: the k the estimated normals were built with (0: none yet)
	Buf<float4> d_src_normals_;                           // N, the source's order; grow-only
	double source_normal_build_ms_ = 0;
	// generalized ICP (opt-in): the flag and its epsilon; the source normals are the symmetric form's
	bool icp_generalized_ = false;
	float gicp_eps_ = 1e-3f;
	bool reads_source_normals() const { return icp_symmetric_ || icp_generalized_; }                 // a flag that reads them is set
	bool source_normals_active() const { return reads_source_normals() && icp_metric_ == 1; }        // and its form is the one every ICP runs
	// launch_icp_iteration_opt's and launch_pose_info's metric where the public one is `metric`
	int kernel_metric(int metric) const { return metric != 1 ? metric : icp_generalized_ ? 3 : icp_symmetric_ ? 2 : 1; }
	int icp_kernel_metric() const { return kernel_metric(icp_metric_); }
	// what the two flags' setters share: the refusals, the flags' new values, the source normals and the form's first launch
	void set_normal_form(const char* fn, bool enabled, bool symmetric, bool generalized, float epsilon, int source_normal_k);
	void ensure_source_normals();
	// launch_estimate_normals on the source in the caller's point order, then the gather into the source's order.  d_xyz / d_perm: the cloud and
	// the permutation where they are on the device already (a swap), else both are uploaded
	void build_source_normals(const float* h_xyz, const float* d_xyz, const int32_t* d_perm);
	void check_swap_size(size_t n, const char* fn) const;   // a swap to fewer than source_normal_k points is refused while either flag is on
	// pose information (allocated on first use, grown on demand): one accumulator block (kIcpBatchAccWords) and one argument block per pose
	Buf<unsigned long long> d_info_acc_; Buf<PoseInfoArgs> d_info_args_;
	double src_crad_ = -1.0;           // largest distance of a source point from the source centroid (first use)
	void ensure_pose_info(size_t K);
	const goicp_comm_ops* icp_comm_ = nullptr;
	bool unrefined_ = false;           // collective registration: the best pose is an upper bound not yet refined by ICP
	// nn query staging grows on demand
	float rot_coeff_[20];

	// search state
	std::priority_queue<Node> queue_;
	float opt_err_ = 1e10f;
	float optR_[9], optT_[3], curR_[9], curT_[3];
	bool early_exit_ = false, converged_ = false;
	int rot_ramp_ = 8;
	void prune_queue();               // drop queued nodes that can no longer win (jly_goicp.cpp:533-543)
	Counters cnt_;
	std::atomic<bool> cancel_{false};
	std::mutex mtx_;
	Result snap_{};
	double dt_build_ms_ = 0, register_ms_ = 0, bnb_ms_ = 0, icp_ms_ = 0, t_submit_ = 0, t_wait_ = 0, t_collect_ = 0;
	long long level_hist_[32] = {};   // verbose: translation expansions by parent depth
	// icp_step state
	float stepR_[9], stepT_[3];
};

// ---- host utilities (config_io.cpp, kdtree.cpp) ----
struct KdHost {
	std::vector<std::vector<float>> boxes;   // per level: groups x 384 floats (level 0: the root; level l: F*64^(l-1) groups, F = real children of the root)
	std::vector<float4> pts;                 // kLeafSlots slots per leaf
	int K = 1, L = 64;
};
void build_kdtree(const float* xyz, int M, int leaf_max, KdHost* out);
// fn(0..ntasks-1) on up to `threads` host threads (tasks claimed from a counter; the first exception is rethrown)
void parallel_tasks(int threads, int ntasks, const std::function<void(int)>& fn);
void rodrigues(float ax, float ay, float az, float R[9]);   // jly_goicp.cpp:449-467
// goicp_source_order_host: the source order of Params::morton_sort on the host (kdtree.cpp); perm[sorted position] = original index
void source_order_host(const float* xyz, size_t n, int mode, int32_t* perm);
// per-axis minimum and largest extent (at least 1e-30) of a cloud, as the Morton order quantises it
void source_morton_frame(const float* xyz, size_t n, float mn[3], float* ext);
// voxel-grid downsampling (kdtree.cpp).  voxel_frame checks the cloud and the voxel (std::invalid_argument: empty or too large a
// cloud, a non-finite coordinate, a voxel that is not positive and finite, extent / voxel >= 2^21) and fills what both paths share;
// voxel_downsample_host is goicp_voxel_downsample_host: out_xyz holds 3 n floats, out_count (may be null) n ints
void voxel_frame(const float* xyz, size_t n, float voxel, VoxelFrame* f);
void voxel_downsample_host(const float* xyz, size_t n, float voxel, float* out_xyz, int32_t* out_count, size_t* m);
// radius outlier removal (kdtree.cpp).  radius_check_params refuses what needs no cloud (std::invalid_argument: a radius that is
// not positive and finite or whose square is no normal float, min_neighbors < 1); radius_frame checks those and the cloud (what voxel_frame
// refuses, extent / radius >= 2^16) and fills the frame of the grid of pitch radius * 1.03125f; radius_frame_of_box is the same from the
// per-axis bounds of a cloud the host has not seen.  radius_outlier_removal_host is goicp_radius_outlier_removal_host: out_xyz holds 3 n
// floats, out_index (may be null) n ints, out_count (may be null) n ints
void radius_check_params(float radius, int32_t min_neighbors);
void radius_frame(const float* xyz, size_t n, float radius, int32_t min_neighbors, VoxelFrame* f);
void radius_frame_of_box(const float mn[3], const float mx[3], size_t n, float radius, int32_t min_neighbors, VoxelFrame* f);
void radius_outlier_removal_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, float* out_xyz, int32_t* out_index,
                                 int32_t* out_count, size_t* m);
// Euclidean / DBSCAN clustering (kdtree.cpp).  cluster_frame / cluster_frame_of_box are radius_frame / radius_frame_of_box with
// min_neighbors == 0 legal and a negative one refused; cluster_check_select refuses a negative min_size or max_clusters; cluster_select is
// the selection over the c sizes that both paths share (keep[l] = 1 or 0).  cluster_host / cluster_filter_host are goicp_cluster_host /
// goicp_cluster_filter_host
// RANSAC plane segmentation (kdtree.cpp).  plane_check_cloud refuses an empty, too large or non-finite cloud; plane_check_select
// what goicp_segment_plane refuses of the parameters, and returns them with the defaults filled in.  segment_plane_host is
// goicp_segment_plane_host and goicp_plane_filter_host in one: every output may be null
void plane_check_cloud(const float* xyz, size_t n);
PlaneSelect plane_check_select(float distance, int32_t iterations, int32_t refine, int32_t max_planes, int32_t min_inliers, uint64_t seed);
void segment_plane_host(const float* xyz, size_t n, const PlaneSelect& s, int32_t* out_label, float* out_xyz, int32_t* out_index, PlaneRecord* out_planes,
                        size_t* n_planes, size_t* m);
// RANSAC pose estimation from correspondences (kdtree.cpp).  ransac_pose_check_select / ransac_pose_check_input refuse what
// goicp_ransac_pose refuses of the parameters (and return them with the defaults filled in) and of the clouds and correspondences;
// ransac_pose_frame is the refit's frame of one side (0 source, 1 target); ransac_pose_host is goicp_ransac_pose_host (out_inlier may be
// null) and select_matches_host goicp_select_matches
RansacPoseSelect ransac_pose_check_select(float distance, int32_t iterations, int32_t refine, int32_t max_poses, int32_t min_inliers, float edge_similarity,
                                          uint64_t seed);
void ransac_pose_check_input(const float* src, size_t n_s, const float* tgt, size_t n_t, const int32_t* corr, size_t M);
void ransac_pose_frame(const float* xyz, const int32_t* corr, size_t M, int side, RansacPoseFrame* f);
void ransac_pose_host(const float* src, const float* tgt, const int32_t* corr, size_t M, const RansacPoseSelect& s, RansacPoseRecord* out_poses, size_t* n_poses,
                      uint8_t* out_inlier);
void select_matches_host(const int32_t* index, const float* d2, const float* d2_second, const uint8_t* mutual, size_t n_q, float ratio, int32_t require_mutual,
                         int32_t* out_corr, size_t* M);
void cluster_frame(const float* xyz, size_t n, float radius, int32_t min_neighbors, VoxelFrame* f);
void cluster_frame_of_box(const float mn[3], const float mx[3], size_t n, float radius, int32_t min_neighbors, VoxelFrame* f);
void cluster_check_select(int32_t min_size, int32_t max_clusters);
void cluster_select(const int32_t* sizes, size_t c, int32_t min_size, int32_t max_clusters, std::vector<int32_t>* keep);
void cluster_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t* out_label, int32_t* out_sizes, size_t* n_clusters);
void cluster_filter_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t min_size, int32_t max_clusters, float* out_xyz,
                         int32_t* out_index, int32_t* out_label, size_t* m);
// statistical outlier removal (kdtree.cpp).  stat_check_params refuses neighbors outside 1..64 or above n - 1 and a std_ratio that
// is negative, NaN or infinite; stat_check_cloud what voxel_frame refuses of a cloud, and returns its per-axis bounds.  stat_levels is the
// plan both paths search by: r0 (0 = no grid level, the top level alone) and the number of grid levels at radii r0 * 2^L, fixed in advance
// from the extent, n, k and a sample of the cloud (ns = stat_sample_size(n) points, every (n / ns)-th; may be null), which only steers the
// amount of work.  statistical_outlier_removal_host is goicp_statistical_outlier_removal_host
void stat_check_params(size_t n, int32_t neighbors, float std_ratio);
void stat_check_cloud(const float* xyz, size_t n, float mn[3], float mx[3]);
size_t stat_sample_size(size_t n);
void stat_levels(const float mn[3], const float mx[3], size_t n, int32_t neighbors, const float* sample, size_t ns, float* r0, int* levels);
void statistical_outlier_removal_host(const float* xyz, size_t n, int32_t neighbors, float std_ratio, float* out_xyz, int32_t* out_index,
                                      float* out_mean_dist, double* threshold, size_t* m);
// exact self k-NN and normal estimation (kdtree.cpp).  knn_self_check_params refuses k outside 1..32 or above n - 1,
// normals_check_params k outside 3..32, k - 1 above n - 1 and a non-finite viewpoint; the cloud is checked by stat_check_cloud.
// knn_self_host / estimate_normals_host are goicp_knn_self_host / goicp_estimate_normals_host
void knn_self_check_params(size_t n, int32_t k);
void normals_check_params(size_t n, int32_t k, const float* vp);
void knn_self_host(const float* xyz, size_t n, int32_t k, int32_t* out_index, float* out_dist_sq);
void estimate_normals_host(const float* xyz, size_t n, int32_t k, const float* vp, float* out_normals, float* out_variation, int32_t* out_index);
// FPFH descriptors and descriptor matching (kdtree.cpp).  fpfh_check_normals refuses null and non-finite normals,
// match_check_descriptors empty, oversized and non-finite descriptor sets; the cloud and k are checked as the self k-NN checks them.
// fpfh_host / match_features_host are goicp_fpfh_host / goicp_match_features_host
void fpfh_check_normals(const float* normals, size_t n);
void match_check_descriptors(const float* q, size_t nq, const float* t, size_t nt);
void fpfh_host(const float* xyz, const float* normals, size_t n, int32_t k, float* out_fpfh, uint8_t* out_spfh_counts);
void match_features_host(const float* q, size_t nq, const float* t, size_t nt, int32_t* out_index, float* out_d2, float* out_d2_second, uint8_t* out_mutual);
// goicp_information_decompose: cyclic Jacobi of the symmetrised 6x6, rank and pseudo-inverse over the eigenvalues > rank_tol * lambda_max (engine.cpp)
void information_decompose(const double info[36], double rank_tol, double eig[6], double vec[36], double pinv[36], int32_t* rank);
void debug_kabsch(const float H[9], float R[9]);            // the device SVD routine on the current device (tests)

}  // namespace goicp
