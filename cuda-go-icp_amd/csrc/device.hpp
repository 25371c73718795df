// Device layer of the MI355X Go-ICP engine: plain structs + launch wrappers (implemented in
// device.hip, compiled by hipcc for gfx950).  Host C++ (engine.cpp, goicp_api.cpp) only sees this.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/goicp_mi355.h"   // GOICP_FPFH_COS / GOICP_FPFH_SIN: the one table of the host path and the kernel

namespace goicp {

// Search-range cull shared by the host queues (engine.hpp) and the device queues (bnbqueue.hip): the half-open cube
// [x, x+w)^3 against the closed range [lo, hi] -- low face of the range exclusive for a cube that only ends there,
// high face inclusive for the cube that starts there ([params.rotation] / [params.translation] of the reference's
// configs, src/common.h:157-169).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool cube_in_range(float x, float y, float z, float w, const float lo[3], const float hi[3])
{
	return x + w > lo[0] && x <= hi[0] && y + w > lo[1] && y <= hi[1] && z + w > lo[2] && z <= hi[2];
}

// Layout 1's order inside a 4x4x4 brick: x fastest (16-B x rows), then y, then z: element = x&3 | (y&3)<<2 | (z&3)<<4.  The parts
// are per axis, so offsets stay separable: element = brick_x(x) | brick_y(y) | brick_z(z).  (4x2x2-voxel 64-B sectors cut the
// modelled tag lookups of the headline batch by 8 % -- tools/dt_sector_model.py -- but measured 0.7 % slower: more index arithmetic.)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned brick_x(unsigned x) { return x & 3u; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned brick_y(unsigned y) { return (y & 3u) << 2; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned brick_z(unsigned z) { return (z & 3u) << 4; }
// element index of voxel (x, y, z) in a bricked grid of VB bricks per side
#if defined(__HIPCC__)
__host__ __device__
#endif
inline size_t brick_index(size_t x, size_t y, size_t z, size_t VB)
{
	return (((z >> 2) * VB + (y >> 2)) * VB + (x >> 2)) * 64 + (brick_x((unsigned)x) | brick_y((unsigned)y) | brick_z((unsigned)z));
}

// Distance transform of the target cloud, resident in HBM.
//   layout 0: linear  [z][y][x], x fastest                       (reference order, jly_3ddt.h:53-79)
//   layout 1: bricked 4x4x4 voxels per 256-B brick, bricks [bz][by][bx], voxels [z][y][x] (brick_index); a surface patch
//             touched by one wavefront then spans ~4x fewer cache lines than in the linear layout
//   layout 2: the bricked grid in half precision (128-B bricks), rounded toward zero; bounds evaluation only, opt-in
struct DtDesc {
	const float* grid;
	int V;          // voxels per side
	int VB;         // bricks per side = ceil(V/4)         (layout 1)
	int layout;
	// truncation distance g of the search objective (goicp_set_search_truncation; 0 = off).  > 0: the bound launches (launch_bounds*, launch_bounds_queue,
	// launch_bounds_tile*) pick their TRUNC instantiations, which clamp every term at g (device.hip trunc_clamp); nothing else reads it.  It sits in
	// what was the padding in front of `scale`: the struct, and with it the argument block of every kernel, keeps its size and offsets
	float trunc;
	double scale;   // voxels per unit                      (jly_3ddt.cpp:923)
	double xmin, ymin, zmin;
	// float images of the geometry + the error model of the float index fast path (device.hip voxel_fast)
	float scale_f, xmin_f, ymin_f, zmin_f;
	float c1, c2;   // |F_float - F_exact| <= c1 + c2*|F|
	const double* overshoot;   // [n_overshoot]: (double)sqrtf(s)/scale for the out-of-grid extension (jly_3ddt.cpp:1025)
	int n_overshoot;
	// nearest-target-point table (ICP only; null = absent): per voxel, in the grid's layout, the leaf slot (KdDesc::pts) of a
	// target point whose seed voxel is nearest to this voxel -- a REAL candidate for the neighbour search of any query that
	// falls into the voxel, i.e. an upper bound that is almost always the answer itself (launch_nn_seed_build)
	const int32_t* nn_ids;
};
static_assert(sizeof(DtDesc) == 104 && offsetof(DtDesc, trunc) == 20 && offsetof(DtDesc, scale) == 24, "DtDesc layout");

// One translation sub-cube to bound (the inner body of GoICP::InnerBnB, jly_goicp.cpp:262-315).
struct CubeRec {
	float tx, ty, tz;   // cube centre  (jly_goicp.cpp:271-273)
	float delta;        // translation uncertainty radius sqrt(3)/2*w (jly_goicp.cpp:263)
	float coeff;        // rotation uncertainty coefficient 2*sin(min(sqrt3*sigma_l,pi)/2), 0 for the ub pass
	int32_t rot;        // index into the rotation table
};
static_assert(sizeof(CubeRec) == 24, "CubeRec layout");

// One BnB expansion: the kernels derive the 8 children themselves (same float operations as the host,
// jly_goicp.cpp:262-273), so the search driver uploads 24 B per expansion instead of 192.
struct ParentRec {
	float x, y, z;      // parent cube corner
	float w;            // parent cube width
	float coeff;        // rotation uncertainty coefficient of the children, 0 for the ub pass
	int32_t rot;        // index into the rotation table
};
static_assert(sizeof(ParentRec) == 24, "ParentRec layout");

struct Rot9 { float r[9]; };   // row-major

// Flattened k-d tree over the target cloud.  The host builds a balanced binary k-d
// tree by median splits and flattens it into a 64-ary hierarchy of tight bounding boxes with K
// levels (branching factor = wavefront width): group g of level l holds its 64 children's boxes as
// six runs of 64 floats {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z} (384 floats); level l has 64^l groups;
// the children of group g are groups 64g .. 64g+63 of level l+1, or, on the last level, leaves.
// Leaf f owns the kLeafSlots consecutive float4 slots pts[kLeafSlots*f ...] (one aligned 256-B block);
// unused slots hold +inf coordinates with index INT_MAX, empty children have inverted infinite boxes.
constexpr int kLeafSlots = 16;
constexpr int kMaxLevels = 3;
struct KdDesc {
	const float* boxes[kMaxLevels];  // boxes[l]: 64^l groups x 384 floats
	const float4* pts;               // [kLeafSlots * 64^K]  leaf order; .w = original index (int bits)
	int K;                           // levels: 64^K leaves
	int M;
};

struct Pose { float R[9]; float t[3]; };

constexpr int kGroup = 8;          // cubes per workgroup pass (the 8 siblings of one BnB expansion)
constexpr int kBoundsThreads = 256;
constexpr int kIcpAcc = 16;        // sum(q-cq)[3] sum(m-cm)[3] sum((q-cq)(m-cm)^T)[9] sum(d^2)
// the rank rule of every 6x6 pose matrix: an eigenvalue counts iff it exceeds kIcpRankTol times the largest (the Gauss-Newton solve of
// the opt-in ICP iterations, pose_information's default)
constexpr double kIcpRankTol = 1e-6;
// a point-to-point covariance H whose largest entry is within kIcpCovNoise of sum |q - cq|^2 + sum |m - cm|^2 is the rounding of its own terms
// and is taken as 0 (finalize_rows)
constexpr double kIcpCovNoise = 0x1p-20;

// ---- bounds ---------------------------------------------------------------------------------
// scratch must hold groups*chunks*2*kGroup floats.  ub/lb: [B].
size_t bounds_scratch_floats(int B, int N, int* groups_out, int* chunks_out);
// `parents` != nullptr: B/8 expansions, `cubes` ignored
// `bo` given (lean bricked grids, at least bo->min_groups groups): a device pre-pass orders the groups by where their gathers land and the
// launch walks them in that order (mode 1), two neighbours of the order at a time (mode 2); every group writes its own rows: same bits
struct BoundsOrder {
	int mode;                    // 1 order, 2 order + pairs
	int min_groups, max_runs;    // fewer groups, or more runs of equal rotation: the launch is the unordered one
	float cell_vox;              // smallest Morton cell of the order, in DT voxels
	int* alias;                  // [groups], or null (bounds_dedup = 0).  alias[g] = the group of g's run whose eight records equal g's as raw bits and
	                             // that the pre-pass met first (the OWNER; alias[owner] = owner): the pair launch over several chunks evaluates owners
	                             // only and bounds_finalize sums a copy's bounds from its owner's rows.  Valid where ctl[1] = 1
	unsigned* order;             // [groups]
	int* pairs;                  // [2 * bounds_order_items(groups, max_runs)]: the two groups of an item, -1 = none
	int* ctl;                    // [0] items of the pair list, [1] 1 = order and pairs are valid (0: too many runs); [2], [3] items the pair launch
	                             // evaluated in twin form / in identical form (coincident members, bounds_pair_kernel): zeroed by the pre-pass
	                             // [kBoundsCut .. kBoundsCut + 8] the cuts of the pair launch's 8-chunk shape (bounds_cuts), in ctl[0]'s 128-B line
	                             // [kBoundsCopies] groups the pair launch did not evaluate, being copies (alias[g] != g): zeroed by the pre-pass
	long long* host_note;        // pinned host memory: the pre-pass leaves (groups << 1 | left alone) there, a hint for the caller's next launch
	const int* cost;             // [kBoundsCost + kBoundsPlan] lines[8], waves[8] of the source's eight chunks and the plan of the cuts made from
	                             // them (launch_bounds_chunk_cost, bounds_cut_plan); null or balance = 0: equal cuts
	int balance;                 // 1: the cuts follow the chunks' cost
};
constexpr int kBoundsOrderMaxRuns = 64;
constexpr int kBoundsCut = 4, kBoundsCopies = 13, kBoundsCtlInts = 32;     // ctl[] is one 128-B line
constexpr int kBoundsAliasProbes = 32;                 // slots of the pre-pass's table a group looks at before it gives up and stays its own owner
constexpr float kBoundsBalanceA = 18.f;                // default weight of a wavefront, in lines: the fit of the spans, EXPERIMENTS R9.1
inline size_t bounds_order_items(int groups, int max_runs) { return (size_t)(groups + 1) / 2 + (size_t)max_runs; }
// slots per block label of the pair launch's grid: no piece of the cuts is longer than 1.25 items (bounds_cuts clamps the weights)
inline int bounds_pair_slots(int max_items, bool balanced) { return balanced ? (int)(((long long)max_items * 5 + 3) / 4) : max_items; }
// Integer cuts of the U = 8 items units (u = chunk * items + item) into eight pieces of equal weight.  A unit of chunk k weighs
// W_k = a_q8 * waves_k + 256 * lines_k, clamped to [0.8, 1.25] x the mean weight; cut[x] is the first unit at which the weighted prefix reaches
// x / 8 of the total.  Everything is 64-bit integer arithmetic on weights scaled to a mean of 2^20: items = 2^20 gives products below 2^47.
// The work is split by what it depends on.  bounds_cut_plan, once per source cloud and weight (launch_bounds_chunk_cost): the clamped weights
// w[8] and their total, and from them, for x = 1 .. 7, the chunk k_x the cut falls into -- 8 (w_0 + .. + w_k) <= x total is free of `items` --
// and n_x = x total - 8 (w_0 + .. + w_{k - 1}), d_x = 8 w_k: plan[x] = k_x, plan[8 + x] = n_x, plan[16 + x] = d_x (entry 0 unused).
// bounds_cut_of, per batch: cut[x] = k_x items + min(ceil(items n_x / d_x), items), one division.  bounds_cut_cap then enforces the bound of a
// piece.  No cost (a cloud without the 8-chunk shape): k_x = x, n_x = 0, the equal split.
constexpr int kBoundsCost = 16, kBoundsPlan = 24;      // BoundsOrder::cost: lines[8], waves[8], then the plan
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void bounds_cut_plan(const int* cost, int a_q8, int plan[kBoundsPlan])
{
	long long w[8], sum = 0;
	for (int k = 0; k < 8; k++) { w[k] = (long long)a_q8 * cost[8 + k] + 256ll * cost[k]; sum += w[k]; }
	for (int x = 0; x < 8; x++) { plan[x] = x; plan[8 + x] = 0; plan[16 + x] = 1; }
	if (sum <= 0) return;
	while (sum >= (1ll << 39)) { sum = 0; for (int k = 0; k < 8; k++) { w[k] >>= 1; sum += w[k]; } }   // keeps w << 23 inside 63 bits
	long long total = 0;
	for (int k = 0; k < 8; k++) {
		long long s = (w[k] << 23) / sum;                  // 2^20 x the weight over the mean weight
		s = s < 838861 ? 838861 : (s > 1310720 ? 1310720 : s);   // [0.8, 1.25] x 2^20
		w[k] = s; total += s;
	}
	int k = 0;
	long long before = 0;                                   // weight of the whole chunks before k, per item
	for (int x = 1; x < 8; x++) {
		while (k < 7 && 8 * (before + w[k]) <= x * total) { before += w[k]; k++; }
		plan[x] = k; plan[8 + x] = (int)(x * total - 8 * before); plan[16 + x] = (int)(8 * w[k]);     // both below 2^27
	}
}
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int bounds_cut_of(const int* plan, int x, int items)
{
	if (x <= 0) return 0;
	if (x >= 8) return 8 * items;
	const long long d = plan[16 + x];
	long long j = ((long long)items * plan[8 + x] + d - 1) / d;
	if (j > items) j = items;
	return (int)((long long)plan[x] * items + j);
}
// the clamp bounds a piece by 1.25 items but for a corner (an empty chunk raised to 0.8 lifts the mean of the clamped weights: 1.26 items);
// the grid has ceil(1.25 items) slots per label, so the bound is enforced: forward, then back from the fixed end
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void bounds_cut_cap(int cut[9], int items)
{
	const int cap = (int)(((long long)items * 5 + 3) / 4);
	for (int x = 1; x < 8; x++) if (cut[x] > cut[x - 1] + cap) cut[x] = cut[x - 1] + cap;
	for (int x = 7; x >= 1; x--) if (cut[x] < cut[x + 1] - cap) cut[x] = cut[x + 1] - cap;
}
// the whole formula in one piece (the host's restatement of what the two device steps leave in ctl[])
inline void bounds_cuts(const int* cost, int a_q8, int items, int cut[9])
{
	int plan[kBoundsPlan];
	bounds_cut_plan(cost, a_q8, plan);
	for (int x = 0; x < 9; x++) cut[x] = bounds_cut_of(plan, x, items);
	bounds_cut_cap(cut, items);
}
hipError_t launch_bounds(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const CubeRec* cubes, const ParentRec* parents,
                         int B, float* scratch, float* ub, float* lb, hipStream_t stream, const BoundsOrder* bo = nullptr);
// What a chunk of the ordered source costs the pair launch (BoundsOrder::cost), once per source cloud: over the eight chunks of the 8-chunk
// shape (chunk_pts = roundup256(ceil(N / 8)); fewer than 32 x 256 points: all zero, equal cuts) and the four rotations of kCostRots at
// translation 0, per wavefront of 64 consecutive points the distinct 128-B lines of the bricked fp32 grid under its in-grid lanes.
// cost[0..7] lines, cost[8..15] wavefronts counted (one per wavefront and rotation); integer sums, hence the same whatever the order.
// a_q8: the weight of a wavefront in lines, in 1/256; a one-thread kernel behind the count leaves the plan of the cuts in cost[16 ..]
hipError_t launch_bounds_chunk_cost(const float4* src, int N, const DtDesc& dt, int a_q8, int* cost, hipStream_t stream);
constexpr int kXcdStampRows = 16, kXcdStampCols = 6;   // diagnostic build (GOICP_BOUNDS_XCD_STAMPS): rows 0-7 per XCC, 8-15 per block label
// copies the stamps out and clears them; hipErrorNotSupported in the shipped library
hipError_t bounds_xcd_stamps_take(unsigned long long* out, hipStream_t stream);

// an UNRELATED cube batch, evaluated grouped by (rotation, pass, translation cell) and written back in the caller's order (same bits)
size_t bounds_grouped_scratch_bytes(int B, int nrots);
hipError_t launch_bounds_grouped(const float4* src, int N, const DtDesc& dt, const Rot9* rots, int nrots, const CubeRec* cubes, int B, void* group_scratch,
                                 float* scratch, float* ub, float* lb, hipStream_t stream);

// trimmed form: only the `inliers` smallest residuals of each cube are summed (jly_goicp.cpp:293-315)
hipError_t launch_bounds_trim(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const CubeRec* cubes, const ParentRec* parents, int B,
                              int inliers, float* ub, float* lb, hipStream_t stream);

// ---- device-resident inner BnB (bnbqueue.hip): one queue per inner search, rounds without the host --------------
constexpr int kQueueCap = 8192;     // nodes per search queue (a queue that would overflow sends the batch back to the host driver)
constexpr int kQueueMaxPop = 512;   // most expansions per search and round: what a LONE search may list (a round costs ~150 us of launches and barriers whatever it
                                    // lists, so the last searches of a batch take big steps)
constexpr int kQueueRoundPop = 128;  // ... and what the round's lists are sized for per search slot (QParams::kmax keeps the total inside: many searches, small steps)
struct QNode { float x, y, z, w, ub, lb; };                    // corner + width (TRANSNODE, jly_goicp.h:59-72)
struct QSearch {                    // one GoICP::InnerBnB call (jly_goicp.cpp:227-340)
	float best;                     // optErrorT (in: the incumbent; out: the search's value)
	float coeff;                    // rotation uncertainty coefficient of this pass, 0 for the upper-bound pass
	int32_t rot;                    // rotation slot
	int32_t count;                  // queued nodes
	int32_t done, improved;         // done: 1 = finished, 2 = stopped because its queue outgrew the slab (QParams::soft_overflow)
	int32_t n_parents, parent_off;  // this round's expansions in the round's list
	int32_t pops, cubes;            // tNodeCount of this search / children evaluated
	float bx, by, bz, bw;           // best child (corner, width), valid when improved
	int32_t tile;                   // this round's expansions are in the tile list (parent_off counts in that list)
	float min_ub;                   // smallest upper bound of any child this search evaluated (whether or not it beat the incumbent)
	int32_t deep;                   // diagnostics: the last selection lay within the tile spread
	int32_t stale;                  // rounds since this search's incumbent last improved (QParams::stale_widen)
	int32_t twin;                   // the other search of the same rotation child (upper-bound pass <-> lower-bound pass), -1: none.  When both list
	                                // the SAME translation node in a round, the lower-bound pass's work items evaluate it for both (one gather, two
	                                // subtractions): bounds_work, device.hip
};
struct TileSeg { int32_t off, n, rot; };   // tile list: a search's expansions parents[off .. off+n), n <= 64, one rotation
struct QCtl {
	int32_t n_groups[2];            // expansions listed per round parity
	int32_t overflow;
	int32_t chunks;                 // point chunks per expansion of the last bound evaluation: > 1 -> its sums are chunk partials in the scratch block,
	                                // added up by the next round's digest (bnb_queue_kernel) -- no separate finalize launch
	int32_t work[2][8];             // per round parity and XCD slot: next work item of the bound evaluation (dynamic distribution)
	// second expansion list of a round (LDS-staged DT tiles, device.hip bounds_tile_kernel): the searches whose selected nodes lie
	// close together -- a few voxels -- are listed here instead and evaluated from DT boxes staged in LDS
	int32_t n_tile_groups[2];       // expansions in the tile list per round parity
	int32_t n_tile_segs[2];         // segments (<= 64 expansions of one search) per round parity
	int32_t tile_chunks;            // point chunks per segment of the last tile evaluation (its sums are chunk partials when > 1)
	int32_t tile_hint;              // running count of (search, round) pairs that qualified for the tile list, whether it was on or not
	int32_t tile_total;             // running count of expansions listed in the tile list
	int32_t n_active[2];            // searches that listed expansions, per round parity (exact: the host sizes the next rounds' steps by it)
	int32_t sel_hist[4][4];         // diagnostics (verbose): expansions selected, by [selection size < 16, < 32, < 64, >= 64][spread <= 5, <= 10, <= 20, > 20 voxels]
};
struct QTile {                      // buffers of the tile list (all null / zero: tiles off)
	ParentRec* parents[2];
	TileSeg* segs[2];
	float* ub; float* lb; float* scratch;
};
struct QParams {
	float thr;                      // SSEThresh
	int32_t K;                      // expansions per search and round (<= kQueueMaxPop)
	int32_t kmax;                   // cap on K after the kernel's own widening: searches still running x kmax fits the round's lists
	int32_t list_cap;               // expansions the round's lists hold (a round that would exceed it flags overflow: host fallback)
	int32_t seg_cap;                // segments the tile list holds (list_cap / 64 + search slots: every search adds at most one partial segment)
	float root_x, root_y, root_z, root_w;
	int32_t boxed, depth;           // translation range culling / depth limit (0 = none)
	int32_t cap;                    // nodes a queue may hold (<= kQueueCap; smaller values only to exercise the overflow path)
	int32_t soft_overflow;          // 1: a search whose queue outgrows its slab stops with QSearch::done = 2 and the others go on (the host re-runs that search
	                                // alone through its own queues); 0: it raises QCtl::overflow and the whole batch goes back
	float lo[3], hi[3];
	int32_t tile_on;                // 1: searches that qualify are listed in the tile list this round (its evaluation is launched)
	int32_t tile_min;               // fewest expansions for the tile list (a lane group of the tile kernel = one expansion)
	float tile_spread;              // largest extent, per axis, of the selected nodes' translations (world units) for the tile list
	int32_t stale_widen;            // 1: a search whose incumbent did not improve in its last round expands up to 2 K nodes, after three such rounds 4 K (<= kQueueMaxPop and QParams::kmax)
	int32_t stale_compact;          // > 0: such a search takes its nodes in Morton order (compact, depth-first-like) once its queue holds this many (bnbqueue.hip)
	int32_t tile_stats;             // 1: fill QCtl::sel_hist (verbose runs)
	float tile_stats_scale;         // voxels per world unit
};
hipError_t launch_bnb_init(QSearch* searches, QNode* q, int nsearch, const QParams& qp, QCtl* ctl, hipStream_t stream);
// footprint-ordered work items of the bound evaluation (device.hip): buffers and shape of the sorted launch
struct QSort {
	const float4* cen;              // centroid of every chunk of chunk_pts points
	unsigned* keys;                 // per item: Morton cell of the item's footprint centre
	unsigned* hist;                 // 32 768 bins
	unsigned* order;                // the items in bucket order; nullptr = feature off
	int32_t chunk_pts, chunks;      // the sorted launch shape
	int32_t min_groups;             // smaller rounds keep the unsorted shape
	int32_t shift;                  // voxel -> cell
};
struct QInit { int32_t slot; float best; float coeff; int32_t rot; int32_t twin; };
hipError_t launch_bnb_init_list(QSearch* searches, QNode* q, const QInit* d_list, int n, const QParams& qp, hipStream_t stream);
// digest the previous round (prev_parents + ubs/lbs), select this round's expansions into `parents`, count them in ctl->n_groups[parity]
hipError_t launch_bnb_queue(QSearch* searches, QNode* q, int nsearch, const QParams& qp, const ParentRec* prev_parents, ParentRec* parents,
                            const float* ubs, const float* lbs, const float* scratch, QCtl* ctl, int parity, hipStream_t stream, const QTile* tile = nullptr,
                            int* parent_search = nullptr,        // parent_search[g] = the search that listed expansion g of the direct list (for the twin test)
                            bool deep = true);                   // deep: the 64-VGPR build (two searches per CU; batches of a prove-the-optimum run), else the 128-VGPR one (no spills)
// bounds of the tile list of round `parity` (segment count known to the device only); fixed grid
hipError_t launch_bounds_tile_queue(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const QTile& tile, QCtl* ctl, int parity, hipStream_t stream);
size_t bounds_tile_queue_scratch_floats(int max_groups);
int bounds_tile_queue_grid();         // workgroups of that launch (its items walk the grid in a stride loop)
// bounds of the 8 children of the *d_groups expansions in `parents` (count known to the device only); max_groups sizes the grids
// (d_chunks: QCtl::chunks -- the evaluation leaves chunk partials in `scratch` when it splits the cloud, and says so there)
hipError_t launch_bounds_queue(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const ParentRec* parents, const int* d_groups,
                               int* d_work8, int* d_chunks, int max_groups, int inliers, float* scratch, float* ub, float* lb, hipStream_t stream,
                               const QSearch* searches = nullptr, const int* parent_search = nullptr,    // both given: twin expansions are evaluated once
                               const QSort* qsort = nullptr);                                           // given: a round of >= min_groups expansions walks its items in the order launch_queue_sort left
size_t bounds_queue_scratch_floats(int max_groups, int sorted_chunks = 0);
hipError_t launch_chunk_centroids(const float4* src, int N, int chunk_pts, float4* cen, hipStream_t stream);
hipError_t launch_queue_sort(const ParentRec* parents, const Rot9* rots, const int* d_groups, int max_groups, const QSort& qs, const DtDesc& dt, hipStream_t stream);
int qsort_shift(int V);
bool bounds_uses_lean(const DtDesc& dt);      // the launch picks the lean sibling path (and with it twin fusion and footprint-ordered items) for this grid
size_t qsort_hist_bytes();
// LDS-staged DT tiles for the deep expansions of a search (device.hip bounds_tile_kernel): nseg segments of n <= 64 expansions,
// segs = nseg x {int off, int n, int rot}; stats (may be null): [0] sub-patches staged, [1] sub-patches whose box did not fit
hipError_t launch_bounds_tile(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const ParentRec* parents, const void* segs, int nseg, int n,
                              int chunks, float* scratch, float* ub, float* lb, unsigned* stats, hipStream_t stream);

// ---- ICP ------------------------------------------------------------------------------------
// Device-resident state of the ICP loop (ICP3D<float>::Run, jly_icp3d.hpp:181-295).  One
// iteration = icp_pass_kernel (transform, exact 1-NN, pivoted sums) + icp_finalize_update
// (double-precision reduction, convergence test, SVD, pose update); iterations can be queued
// back-to-back, a converged state turns the remaining launches into no-ops.
struct IcpState {
	float R[9], t[3];            // current pose
	float mu_m[3], mu_d[3];      // means carried across iterations (jly_icp3d.hpp:205-206,244-263)
	float cq[3], cm[3];          // pivots of the next pass (current centroids)
	float src_centroid[3];
	float err, err_new;          // previous / last pass: sum of squared NN distances
	float err_diff_n;            // err_diff * num (jly_icp3d.hpp:255)
	float n;                     // number of source points
	int32_t converged, iters, passes;
	int32_t carry_means;         // 1: the reference's carried means; 0: fresh means (single-step API)
	int32_t frozen;              // 1: passes only score, the pose is not updated
	float acc_scale, acc_inv;    // small clouds: the pass adds its sums as 64-bit fixed point, value * acc_scale (a power of two chosen from the
	                             // clouds' extent so that N terms cannot overflow), into kIcpAccReplicas x 16 accumulators
	// distance-gated ICP (goicp_set_icp_gate; all zero and never read without a gate)
	float g2;                    // squared maximum correspondence distance: a correspondence is an inlier iff d^2 <= g2
	int32_t min_inliers;         // fewer inliers in a pass: the pose stays and the loop stops
	int32_t n_in;                // inliers of the last pass
	float cost;                  // truncated cost err + (n - n_in) * g2 of the previous pass: what the stop rule compares (-1: none yet)
	// robust-kernel ICP (goicp_set_icp_robust; all zero and never read without a kernel).  `cost` above is then the robust cost
	// C = sum rho of the previous pass, and `min_inliers` the weight floor (3 / 6)
	int32_t rk;                  // kernel: 1 Huber, 2 Cauchy, 3 Geman-McClure, 4 Tukey
	float rc;                    // scale c > 0
	float w_sum;                 // W = sum of the weights of the last pass
	float cost_new;              // C of the last pass
};
constexpr int kIcpAccReplicas = 32;   // workgroup b adds to replica b % 32: ~60 adds per address and pass (a device-scope atomic takes ~12 ns)
constexpr int kIcpStridedMaxN = 40000;   // up to this many source points: strangers per wavefront + fixed-point sums (device.hip icp_pass_kernel)
int icp_blocks(int N);           // workgroups per pass
size_t icp_partials_floats(int N);   // floats the `partials` buffer of launch_icp_iteration must hold
// ticket: a device int that is zero between launches -> ONE fused launch (the last workgroup to arrive runs the
// finalize); nullptr -> two launches (pass, finalize).  Same arithmetic and summation order: bit-identical states.
// nn_cache: 2 float4 per source point, zero-initialised once (never invalidated: its entries are statements about the
// static target cloud) -> a pass skips, exactly, the tree walk of every query whose cached neighbour is provably still the
// nearest; nullptr -> every query walks.
// acc: kIcpAccReplicas x 16 zeroed 64-bit words (kept zero between iterations by the finalize) -> clouds of up to kIcpStridedMaxN
// points sum there instead of writing a row of partial sums per workgroup; nullptr -> rows for every size
hipError_t launch_icp_iteration(const float4* src, int N, IcpState* d_state, const KdDesc& kd, const DtDesc& dt,
                                float* partials, int* ticket, float4* nn_cache, int* hit_counter, hipStream_t stream, unsigned long long* acc = nullptr);
// The sharded ICP loop (goicp_icp_run_collective), fixed-point form only (bricked DT, acc != nullptr).  One iteration on a rank:
//   launch_icp_pass_slice    the pass over workgroups [b0, b1) of the world-1 grid (icp_blocks(N)) with the global N: every workgroup forms
//                            the float row sums of the same 16 queries as at world 1; no finalize.  b0 == b1: nothing is launched
//   launch_icp_acc_export    one wavefront: the replicas -> 16 int64 totals (replicas zeroed) + the state's converged flag -> out[0..16],
//                            the loop state itself behind them (out + 17): ONE read-back per iteration
//   launch_icp_finalize_from_sums  the totals summed over the ranks (16 int64) -> (double)x * acc_inv -> the update of icp_finalize_update_acc
hipError_t launch_icp_pass_slice(const float4* src, int N, int b0, int b1, IcpState* d_state, const KdDesc& kd, const DtDesc& dt, unsigned long long* acc,
                                 float4* nn_cache, int* hit_counter, hipStream_t stream);
hipError_t launch_icp_acc_export(unsigned long long* acc, const IcpState* d_state, long long* out, hipStream_t stream);   // out: kIcpExportWords
hipError_t launch_icp_finalize_from_sums(const long long* sums16, IcpState* d_state, hipStream_t stream);
constexpr int kIcpExportWords = 17 + (int)((sizeof(IcpState) + 7) / 8);   // launch_icp_acc_export: totals, converged flag, then the loop state
long long icp_slice_queries(int N, int b0, int b1);                      // source points the workgroups [b0, b1) of a pass evaluate
// trimmed iteration: only the `num` nearest correspondences enter the sums (IcpState.n must be num)
int icp_trim_blocks(int N);
// the trimmed iteration's selection of the num smallest nn_d2 (ties in point order) into include[]: kernel 0 = by size (the
// iteration's choice), 1 = registers (N <= 32 768, else hipErrorInvalidValue without a launch), 2 = streaming
hipError_t launch_icp_select(const float* nn_d2, int N, int num, const IcpState* st, unsigned char* include, int kernel, hipStream_t stream);
hipError_t launch_icp_iteration_trim(const float4* src, int N, int num, IcpState* d_state, const KdDesc& kd, const DtDesc& dt,
                                     float* nn_d2, int* nn_slot, unsigned char* include, float* partials, hipStream_t stream);
// In-place p <- R p + t, norm recomputed (ICP::kdTreeGPUStep's kernTransform, icp_kernel.cu:138-144)
hipError_t launch_transform(float4* src, int N, const Pose& pose, hipStream_t stream);
// NN operator on arbitrary queries (kernKDSearchNearest, icp_kernel.cu:146-157)
hipError_t launch_nn_query(const float* q_xyz, int n, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2,
                           hipStream_t stream);

// ---- point-to-plane ICP (opt-in, goicp_set_icp_options) ---------------------------------------------------------------------
constexpr int kKnnMax = 32;        // most neighbours of the k-NN walk (two list entries per lane of a 16-lane row)
constexpr int kIcpPlaneTerms = 28; // upper triangle of J J^T (21), J r (6), d^2
constexpr int kIcpPlaneStride = 32; // accumulator words per replica (28 used)
// exact k-NN of n queries (1 <= k <= min(kKnnMax, M), else hipErrorInvalidValue): idx / d2 are n x k, ascending (d2, original index)
hipError_t launch_knn_query(const float* q_xyz, int n, int k, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2, hipStream_t stream);
// target normals, one float4 per target point in original order (M; the leaf slots of kd.pts are walked): the k nearest target points (the point included),
// fp64 covariance about their mean, eigenvector of the smallest eigenvalue, oriented away from `centroid`; degenerate -> 0.
// target_xyz: the M target points in original order on the device
hipError_t launch_normal_build(const float* target_xyz, int nslots, int k, const float centroid[3], const KdDesc& kd, const DtDesc& dt, float4* normals,
                               hipStream_t stream);

// ---- distance-gated ICP (opt-in, goicp_set_icp_gate) ------------------------------------------------------------------------------
// A gated iteration of either metric (0 point-to-point, 1 point-to-plane; bricked DT only; launch_icp_iteration_opt, kIcpModeGate): the
// metric's pass in its GATE form -- the owning lane of a query contributes its terms and 1 to a count iff d^2 <= IcpState::g2 -- and the
// metric's one-wavefront finalize with the count in place of n and the truncated-cost stop rule.  Fixed-point sums at every N.
constexpr int kIcpGateCountWord[2] = {16, 28};
// goicp_eval_correspondences: the pass's transform (jly_icp3d.hpp:222-224 order) and walk for every source point, one launch;
// idx[i] = original index of the neighbour of source slot i (-1 when d2[i] > g2), d2[i] = the walk's distance bits
hipError_t launch_eval_correspondences(const float4* src, int N, const Pose& pose, float g2, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2,
                                       hipStream_t stream);

// ---- robust-kernel ICP (opt-in, goicp_set_icp_robust) -----------------------------------------------------------------------------
// An IRLS iteration of either metric (bricked DT only; launch_icp_iteration_opt, kIcpModeRobust): the metric's pass in its ROBUST form -- the
// owning lane of a query forms the weight w of IcpState::rk / rc from its residual in float (robust_terms) and multiplies every term of the
// update by it; d^2 stays unweighted -- and the metric's one-wavefront finalize with W = sum w in place of n and the stop rule on C = sum rho.
// Fixed-point sums at every N.
// kIcpRobustWScale: w <= 1, so a workgroup's float row sum is <= 16 and the total over N <= 2^23 points <= 2^23; times 2^36 that is
// 2^59 < 2^63.  A sum of weights that are all 1.0f is an integer and stays exact: W == N.
constexpr double kIcpRobustWScale = 68719476736.0;   // 2^36

// ---- the opt-in ICP iterations: point-to-plane, gate, robust kernel; single pose and batched multi-start (goicp_icp_run_batch) ----
// One iteration (the pass + the one-wavefront finalize) of every cell of (metric, mode, single pose | batch) but the default one -- plain
// point-to-point on a single pose is launch_icp_iteration's.  The linear DT (dt.layout 0) has the plain point-to-plane iteration only.
// Single pose (active == nullptr, n_active == 1): `states` is the device-resident loop state, `acc` kIcpAccReplicas x kIcpPlaneStride zeroed 64-bit
// words (kept zero between iterations by the finalize); the state's acc_scale / acc_inv scale the sums.
// Batch: up to kIcpBatchMax independent loops over the same clouds: states[s] is pose slot s's loop state, acc + s * kIcpBatchAccWords its
// accumulator block (as the single pose's), active[0 .. n_active) the slots this iteration visits (device memory).  Pose s's state evolves bit
// for bit as under the single-pose iteration (launch_icp_iteration(..., acc) for plain point-to-point) on its own.
// The accumulator block, every cell: the replica stride is kIcpPlaneStride words for BOTH metrics but in plain point-to-point (a batch only),
// whose replicas are the default pass's 16 words.  Words 0 .. 15 (metric 0) / 0 .. 27 (metric 1) of a replica are the pass's terms.
//   kIcpModeGate    the inlier count, a plain integer, in word kIcpGateCountWord[metric] = 16 / 28
//   kIcpModeRobust  W (scaled by kIcpRobustWScale) in word kIcpGateCountWord[metric] = 16 / 28, C (scaled by the pass's acc_scale) in the word
//                   after it, 17 / 29
// metric 2 is internal: metric 1 in its symmetric form (goicp_set_icp_symmetric), metric 1's words and modes, src_normals beside normals.
// metric 3 is internal: metric 1 in its generalized form (goicp_set_icp_generalized), likewise, with gicp_eps; an eps outside [kGicpEpsMin, 1] is refused.
constexpr float kGicpEpsMin = 1e-4f;
// Anything else -- a null states or acc, a metric outside 0..3, metric 1 / 2 / 3 without normals, metric 2 / 3 without src_normals, metric 0 or a mode on the linear DT, n_active outside
// [1, kIcpBatchMax] or != 1 without a list, the default cell -- is hipErrorInvalidValue without a launch.
enum IcpMode : int { kIcpModePlain = 0, kIcpModeGate = 1, kIcpModeRobust = 2 };
constexpr int kIcpBatchMax = 1024;
constexpr int kIcpBatchAccWords = kIcpAccReplicas * kIcpPlaneStride;   // accumulator words per slot (either metric)
struct IcpOptArgs {
	const float4* src; int N;
	IcpState* states;             // the loop state; batch: kIcpBatchMax slots at most
	const int* active;            // nullptr: single pose
	int n_active;                 // 1 for a single pose
	int metric;                   // 0 point-to-point, 1 point-to-plane, 2 symmetric point-to-plane, 3 generalized (plane-to-plane)
	int mode;                     // IcpMode
	const float4* normals;        // metric 1: one per target point (launch_normal_build)
	unsigned long long* acc;
	int capped;                   // kIcpModeGate: the walk's pruning bound starts at min(seed distance, g2) -- exact for every inlier, no neighbour for an outlier
	const float4* src_normals = nullptr;   // metric 2 / 3: one per source point, parallel to src (launch_source_normals_gather)
	float gicp_eps = 0.f;                  // metric 3: epsilon, in [kGicpEpsMin, 1]
};
hipError_t launch_icp_iteration_opt(const IcpOptArgs& a, const KdDesc& kd, const DtDesc& dt, hipStream_t stream);

// ---- pose information (goicp_pose_information) -------------------------------------------------------------------------
// One pass at a pose handed in by value: the sums of the Gauss-Newton normal matrix and gradient about the pivot c, of either metric, under the
// weights of a plain (g2 = +inf, rk = 0), gated (g2 finite) or robust (rk != 0, rc) handle.  Bricked DT only.  acc: kIcpAccReplicas x
// kIcpPlaneStride zeroed 64-bit words (the caller zeroes them and adds up the replicas); the first kPoseInfoWords[metric] words of a replica
// are used -- their order: device.hip pose_info_body.  scale: the power of two every word but W (kIcpRobustWScale) and the count is scaled by.
struct PoseInfoArgs {
	float R[9], t[3];
	float c[3];         // pivot
	float g2;           // squared gate, +inf = none
	int32_t rk;         // robust kernel, 0 = none
	float rc;           // its scale
	float scale;        // fixed-point scale of the sums
	float eps;          // metric 3: the generalized form's epsilon (0 elsewhere)
};
static_assert(sizeof(PoseInfoArgs) == 80, "PoseInfoArgs layout");
constexpr int kPoseInfoWords[4] = {19, 31, 31, 31};   // [2], [3]: the symmetric and the generalized form of metric 1 (src_normals beside normals), metric 1's layout
hipError_t launch_pose_info(const float4* src, int N, const PoseInfoArgs& args, int metric, const KdDesc& kd, const DtDesc& dt, const float4* normals,
                            unsigned long long* acc, hipStream_t stream, const float4* src_normals = nullptr);
// n_poses <= kIcpBatchMax argument blocks in device memory, slot s adding into acc + s * kIcpBatchAccWords: each slot the single call bit for bit
hipError_t launch_pose_info_batch(const float4* src, int N, const PoseInfoArgs* d_args, int n_poses, int metric, const KdDesc& kd, const DtDesc& dt,
                                  const float4* normals, unsigned long long* acc, hipStream_t stream, const float4* src_normals = nullptr);
// d_out[i] = (normal of point d_perm[i], 0): normals in the caller's point order (3 n floats) into the source's order
hipError_t launch_source_normals_gather(const float* d_normals_xyz, const int32_t* d_perm, int n, float4* d_out, hipStream_t stream);

// min of n floats (+ first index attaining it, may be null): one workgroup; v must be 16-byte aligned
hipError_t launch_reduce_min(const float* v, int n, float* out_min, int* out_idx, hipStream_t stream);

// ---- test / measurement helpers ---------------------------------------------------------------
hipError_t launch_kabsch_debug(const float* d_H9, float* d_R9, hipStream_t stream);
// window: floats per workgroup window (power of two >= 4096, <= grid size); 8*iters loads per lane
hipError_t launch_probe_gather(const DtDesc& dt, int mode, unsigned window, int blocks, int iters, float* sink, hipStream_t stream);

// ---- device-side build of the box hierarchy (kdbuild.hip): Morton sort + bottom-up boxes ----------
hipError_t launch_kd_build(const float* d_xyz, int M, int K, const float mn[3], float ext, float* const boxes[kMaxLevels],
                           float4* pts, hipStream_t stream);
// ---- source order on the device (kdbuild.hip): the permutation Params::morton_sort defines (goicp_source_order_host is its host twin) ----
// size of the left part when the k-d order splits a run of n points: half, rounded to a multiple of 256 / 64 / 16 / 4 points (the largest
// unit smaller than the run); n <= 1: n (nothing to split).  A function of n alone -- the host recursion and the device levels share it
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int source_order_left(int n)
{
	if (n <= 1) return n;
	const int unit = n > 256 ? 256 : (n > 64 ? 64 : (n > 16 ? 16 : (n > 4 ? 4 : 1)));
	int nl = ((n / 2 + unit / 2) / unit) * unit;
	if (nl == 0) nl = unit;
	if (nl >= n) nl = n - (n % unit ? n % unit : unit);
	return nl;
}
// d_xyz: the n points on the device; mode 0 input order, 1 Morton curve (mn / ext: the cloud's per-axis minimum and largest extent as the
// host forms them), 2 k-d order; d_perm[sorted position] = original index.  Returns after the stream has drained
hipError_t launch_source_order(const float* d_xyz, int n, int mode, const float mn[3], float ext, int32_t* d_perm, hipStream_t stream);
// d_src[i] = (x, y, z, |p|) of point d_perm[i]
hipError_t launch_source_gather(const float* d_xyz, const int32_t* d_perm, int n, float4* d_src, hipStream_t stream);
// ---- voxel-grid downsampling on the device (kdbuild.hip; goicp_voxel_downsample_host is its host twin) ----
// what the host derives from the cloud while it checks it (voxel_frame, kdtree.cpp): the per-axis minimum, the largest offset E from it, the
// shift s of the exact fixed-point terms llrint(ldexp(d, s)), and the number of key bits in use (cell x | y << 21 | z << 42)
struct VoxelFrame {
	float mn[3], E, voxel;
	int s, key_bits;
};
// d_xyz: the n points on the device.  d_out: room for 3 n floats, the first 3 m are written (one centroid per occupied cell, ascending key);
// d_count (may be null): room for n ints, the first m are written.  ev_begin / ev_end (may be null) are recorded around the device work
// proper: the kernels, the read-back of m and the two m-sized allocations, not the n-sized allocations and the frees.  Returns after the
// stream has drained
hipError_t launch_voxel_downsample(const float* d_xyz, int n, const VoxelFrame& f, float* d_out, int32_t* d_count, int* m, hipStream_t stream,
                                   hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// ---- radius outlier removal on the device (kdbuild.hip; goicp_radius_outlier_removal_host is its host twin) ----
// f: the frame of the grid of pitch f.voxel = r * 1.03125f (radius_frame, kdtree.cpp); r2 = r * r in float.  d_out: room for 3 n floats,
// the first 3 m are written (the kept points, input order, own bits); d_index (may be null): room for n ints, the first m are written (the
// kept points' indices, ascending); d_count (may be null): n ints, min(#neighbours, min_neighbors) of every point.  *m may be 0.
// ev_begin / ev_end (may be null) are recorded around the kernels and the read-back of m.  Returns after the stream has drained
hipError_t launch_radius_outlier_removal(const float* d_xyz, int n, const VoxelFrame& f, float r2, int min_neighbors, float* d_out, int32_t* d_index,
                                         int32_t* d_count, int* m, hipStream_t stream, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// ---- Euclidean / DBSCAN clustering on the device (kdbuild.hip; goicp_cluster_host is its host twin) ----
// f: the radius filter's frame (cluster_frame, kdtree.cpp); r2 = r * r in float; min_neighbors >= 0 (0: every point is core).  d_label: n
// ints, the cluster of every point, -1 for noise; d_sizes: room for n ints, the first *c are the clusters' sizes (the rest is zero); *c may
// be 0.  ev_begin / ev_end (may be null) are recorded around the kernels and the read-back of c.  Returns after the stream has drained
hipError_t launch_cluster(const float* d_xyz, int n, const VoxelFrame& f, float r2, int min_neighbors, int32_t* d_label, int32_t* d_sizes, int* c,
                          hipStream_t stream, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// the points whose cluster l has d_keep[l] != 0 (c ints on the device), in input order: d_out room for 3 n floats, d_index and d_out_label
// (each may be null) room for n ints, the first *m written; *m may be 0.  Returns after the stream has drained
hipError_t launch_cluster_compact(const float* d_xyz, int n, const int32_t* d_label, const int32_t* d_keep, float* d_out, int32_t* d_index,
                                  int32_t* d_out_label, int* m, hipStream_t stream, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// ---- statistical outlier removal on the device (kdbuild.hip; goicp_statistical_outlier_removal_host is its host twin) ----
constexpr int kStatMaxLevels = 48;
// what a run did: the grid levels that ran, the points each resolved, and the points left to the top level (all points as candidates)
struct StatReport {
	int levels_run = 0, resolved[kStatMaxLevels] = {}, top = 0;
};
// frames[L] / r2[L], L < levels <= kStatMaxLevels: the frame of the grid of pitch r_L * 1.03125f and r_L * r_L in float, r_L = r0 * 2^L
// (stat_levels and radius_frame_of_box, kdtree.cpp); levels == 0: the top level alone.  k = neighbors in 1..64, k <= n - 1.  d_out: room for
// 3 n floats, the first 3 m are written; d_index (may be null): n ints, the first m are written; d_mean (may be null): n floats, u_i of every
// point; *threshold (may be null): the reported threshold.  *m >= 1.  ev_begin / ev_end (may be null) are recorded around the kernels and
// the read-backs (one int per level, m and the threshold at the end).  Returns after the stream has drained
hipError_t launch_stat_outlier_removal(const float* d_xyz, int n, const VoxelFrame* frames, const float* r2, int levels, int k, float std_ratio,
                                       float* d_out, int32_t* d_index, float* d_mean, double* threshold, int* m, StatReport* report, hipStream_t stream,
                                       hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// ---- exact self k-NN and normal estimation on the device (kdbuild.hip; goicp_knn_self_host / goicp_estimate_normals_host are
// the host twins) ----
constexpr int kKnnSelfMax = 32;
// frames / r2 / levels as launch_stat_outlier_removal takes them.  k in 1..kKnnSelfMax, k <= n - 1.  d_index: n x k ints, row i = the k
// nearest other points of point i ascending by the key (bits of d2) << 32 | index; d_dist_sq (may be null): n x k floats, their d2;
// d_order (may be null): n ints, the points in the order of the first grid level (input order when no level ran).  ev_begin / ev_end (may
// be null) are recorded around the kernels and the read-backs (one int per level).  Returns after the stream has drained
hipError_t launch_self_knn(const float* d_xyz, int n, const VoxelFrame* frames, const float* r2, int levels, int k, int32_t* d_index, float* d_dist_sq,
                           int* d_order, StatReport* report, hipStream_t stream, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// k in 3..kKnnSelfMax counts the point itself, k - 1 <= n - 1.  d_index: n x (k - 1) ints, the neighbours used (launch_self_knn's rows at
// k - 1); vp: the viewpoint on the host, or null; d_normals: n x 3 floats; d_variation (may be null): n floats
hipError_t launch_estimate_normals(const float* d_xyz, int n, const VoxelFrame* frames, const float* r2, int levels, int k, const float* vp,
                                   float* d_normals, float* d_variation, int32_t* d_index, StatReport* report, hipStream_t stream,
                                   hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);

// The PCA of one neighbourhood as include/goicp_mi355.h defines it, one text for the host path (kdtree.cpp) and normal_pca_kernel: fp64,
// every operation rounded once (the device takes the _rn intrinsics, the host is built with -ffp-contract=off), + - * / sqrt only.
#if defined(__HIPCC__)
#define GOICP_HD __host__ __device__
#else
#define GOICP_HD
#endif
namespace pca {
#if defined(__HIP_DEVICE_COMPILE__)
GOICP_HD inline double add(double a, double b) { return __dadd_rn(a, b); }
GOICP_HD inline double sub(double a, double b) { return __dsub_rn(a, b); }
GOICP_HD inline double mul(double a, double b) { return __dmul_rn(a, b); }
GOICP_HD inline double div(double a, double b) { return __ddiv_rn(a, b); }
GOICP_HD inline double root(double a) { return __dsqrt_rn(a); }
#else
GOICP_HD inline double add(double a, double b) { return a + b; }
GOICP_HD inline double sub(double a, double b) { return a - b; }
GOICP_HD inline double mul(double a, double b) { return a * b; }
GOICP_HD inline double div(double a, double b) { return a / b; }
GOICP_HD inline double root(double a) { return std::sqrt(a); }
#endif
GOICP_HD inline double mag(double a) { return a < 0.0 ? -a : a; }
constexpr int kMaxSweeps = 32;

// one Jacobi rotation of the pair (P, Q); false: the pair was skipped
template <int P, int Q> GOICP_HD inline bool rotate(double A[3][3], double V[3][3])
{
	const double app = A[P][P], aqq = A[Q][Q], apq = A[P][Q];
	if (apq == 0.0 || mul(apq, apq) <= mul(1e-24, mag(mul(app, aqq)))) return false;
	const double da = sub(aqq, app), db = add(apq, apq);
	const double tn = div(da >= 0.0 ? db : -db, add(mag(da), root(add(mul(da, da), mul(db, db)))));
	const double cs = div(1.0, root(add(1.0, mul(tn, tn)))), sn = mul(cs, tn);
	for (int k = 0; k < 3; k++) {                                // A <- A G (columns P, Q)
		const double akp = A[k][P], akq = A[k][Q];
		A[k][P] = sub(mul(cs, akp), mul(sn, akq)); A[k][Q] = add(mul(sn, akp), mul(cs, akq));
	}
	for (int k = 0; k < 3; k++) {                                // A <- G^T A (rows P, Q)
		const double apk = A[P][k], aqk = A[Q][k];
		A[P][k] = sub(mul(cs, apk), mul(sn, aqk)); A[Q][k] = add(mul(sn, apk), mul(cs, aqk));
	}
	for (int k = 0; k < 3; k++) {                                // V <- V G
		const double vkp = V[k][P], vkq = V[k][Q];
		V[k][P] = sub(mul(cs, vkp), mul(sn, vkq)); V[k][Q] = add(mul(sn, vkp), mul(cs, vkq));
	}
	return true;
}
}  // namespace pca

// xyz: the cloud; i: the point; row: its kk = k - 1 nearest others in key order; (vpx, vpy, vpz): the viewpoint when has_vp -> the normal and the
// surface variation
GOICP_HD inline void normal_pca_point(const float* xyz, int i, const int32_t* row, int kk, bool has_vp, float vpx, float vpy, float vpz, float out_n[3],
                                      float* out_var)
{
	using namespace pca;
	const double xi = (double)xyz[3 * (size_t)i], yi = (double)xyz[3 * (size_t)i + 1], zi = (double)xyz[3 * (size_t)i + 2];
	const double kd = (double)(kk + 1);
	// the mean of the offsets e_j; the point's own offset (0, 0, 0) comes first
	double sx = 0.0, sy = 0.0, sz = 0.0;
	for (int j = 0; j < kk; j++) {
		const float* q = xyz + 3 * (size_t)row[j];
		sx = add(sx, sub((double)q[0], xi)); sy = add(sy, sub((double)q[1], yi)); sz = add(sz, sub((double)q[2], zi));
	}
	const double mx = div(sx, kd), my = div(sy, kd), mz = div(sz, kd);
	double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
	for (int j = -1; j < kk; j++) {
		double dx = sub(0.0, mx), dy = sub(0.0, my), dz = sub(0.0, mz);
		if (j >= 0) {
			const float* q = xyz + 3 * (size_t)row[j];
			dx = sub(sub((double)q[0], xi), mx); dy = sub(sub((double)q[1], yi), my); dz = sub(sub((double)q[2], zi), mz);
		}
		c00 = add(c00, mul(dx, dx)); c01 = add(c01, mul(dx, dy)); c02 = add(c02, mul(dx, dz));
		c11 = add(c11, mul(dy, dy)); c12 = add(c12, mul(dy, dz)); c22 = add(c22, mul(dz, dz));
	}
	double A[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
	double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
	for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
		const bool r01 = rotate<0, 1>(A, V), r02 = rotate<0, 2>(A, V), r12 = rotate<1, 2>(A, V);
		if (!(r01 || r02 || r12)) break;
	}
	const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
	// the column of the smallest l, the lowest index on equal values (selects on values: an index into V would put it into scratch)
	const bool s1 = l1 < l0;
	const double l01 = s1 ? l1 : l0;
	const bool s2 = l2 < l01;
	const double v0 = s2 ? V[0][2] : (s1 ? V[0][1] : V[0][0]), v1 = s2 ? V[1][2] : (s1 ? V[1][1] : V[1][0]), v2 = s2 ? V[2][2] : (s1 ? V[2][1] : V[2][0]);
	// ascending: a <= b <= c
	double a = l0, b = l1, c = l2, t;
	if (b < a) { t = a; a = b; b = t; }
	if (c < b) { t = b; b = c; c = t; }
	if (b < a) { t = a; a = b; b = t; }
	if (!(c > 0.0)) {                                            // every neighbour coincides with the point
		out_n[0] = out_n[1] = out_n[2] = 0.f;
		*out_var = 0.f;
		return;
	}
	*out_var = (float)div(a > 0.0 ? a : 0.0, add(add(a, b), c));
	const double len = root(add(add(mul(v0, v0), mul(v1, v1)), mul(v2, v2)));
	const float n0 = (float)div(v0, len), n1 = (float)div(v1, len), n2 = (float)div(v2, len);
	double d = 0.0;
	if (has_vp) d = add(add(mul((double)n0, sub((double)vpx, xi)), mul((double)n1, sub((double)vpy, yi))), mul((double)n2, sub((double)vpz, zi)));
	const float lead = n0 != 0.f ? n0 : (n1 != 0.f ? n1 : n2);
	const bool flip = d != 0.0 ? d < 0.0 : lead < 0.f;
	out_n[0] = n0 == 0.f ? 0.f : (flip ? -n0 : n0);
	out_n[1] = n1 == 0.f ? 0.f : (flip ? -n1 : n1);
	out_n[2] = n2 == 0.f ? 0.f : (flip ? -n2 : n2);
}

// ---- FPFH descriptors and descriptor matching (kdbuild.hip; goicp_fpfh_host / goicp_match_features_host are the host twins) ----
constexpr int kFpfhDim = 33, kFpfhBins = 11;
// the matcher's LDS tile: kMatchTile target descriptors, each in a row of kMatchRow words (33 padded to a multiple of four, so that a row
// starts on 16 bytes and is read as eight 128-bit words and one 32-bit word)
constexpr int kMatchTile = 128, kMatchRow = 36;
// frames / r2 / levels as launch_self_knn takes them, k in 1..kKnnSelfMax, k <= n - 1.  d_normals: n x 3 floats; d_index / d_dist_sq: n x k,
// the self k-NN rows (left on the device); d_counts: n x 33 bytes, the SPFH counts; d_fpfh: n x 33 floats.  Returns after the stream has
// drained; ev_begin / ev_end (may be null) are recorded around the search and the two kernels
hipError_t launch_fpfh(const float* d_xyz, const float* d_normals, int n, const VoxelFrame* frames, const float* r2, int levels, int k, int32_t* d_index,
                       float* d_dist_sq, unsigned char* d_counts, float* d_fpfh, StatReport* report, hipStream_t stream, hipEvent_t ev_begin = nullptr,
                       hipEvent_t ev_end = nullptr);
// d_q: nq x 33 floats, d_t: nt x 33 floats; d_index (nq ints), d_d2, d_second (nq floats): the smallest key of every query and the d2 of
// the second smallest (+inf when nt == 1); d_mutual (may be null): nq bytes.  Returns after the stream has drained
hipError_t launch_match_features(const float* d_q, int nq, const float* d_t, int nt, int32_t* d_index, float* d_d2, float* d_second,
                                 unsigned char* d_mutual, hipStream_t stream, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);

// The pair feature and its three bins as include/goicp_mi355.h defines them, one text for the host path (kdtree.cpp) and spfh_kernel: fp64,
// every operation rounded once (pca's + - * / sqrt), comparisons, |.| and floor.
namespace fpfh {
using pca::add; using pca::sub; using pca::mul; using pca::div; using pca::root; using pca::mag;
GOICP_HD inline double dot3(double ax, double ay, double az, double bx, double by, double bz) { return add(add(mul(ax, bx), mul(ay, by)), mul(az, bz)); }
// clamp(floor(11 * ((f + 1) * 0.5)), 0, 10), clamped as a double: f is finite but need not lie in [-1, 1] (the normals need not be unit)
GOICP_HD inline int bin11(double f)
{
	const double t = floor(mul(11.0, mul(add(f, 1.0), 0.5)));
	return t < 0.0 ? 0 : (t > 10.0 ? 10 : (int)t);
}
// the bin of atan2(y, x) among 11 equal bins of [-pi, pi): the number of k in 1..10 with angle(-x, -y) >= 2 pi k / 11
GOICP_HD inline int theta_bin(double x, double y)
{
	if (x == 0.0 && y == 0.0) return 5;
	const double C[10] = GOICP_FPFH_COS, S[10] = GOICP_FPFH_SIN;
	const double a = -x, b = -y;
	int count = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int k = 1; k <= 10; k++) {
		const bool turn = sub(mul(C[k - 1], b), mul(S[k - 1], a)) >= 0.0;
		count += k <= 5 ? (b < 0.0 || turn) : (b < 0.0 && turn);
	}
	return count;
}
// p_i, n_i, p_j, n_j: three floats each -> false: the pair is skipped; true: its bins b[0] (theta), b[1] (f2), b[2] (f3), each in 0..10
GOICP_HD inline bool pair_bins(const float* p_i, const float* n_i, const float* p_j, const float* n_j, int b[3])
{
	double d0 = sub((double)p_j[0], (double)p_i[0]), d1 = sub((double)p_j[1], (double)p_i[1]), d2 = sub((double)p_j[2], (double)p_i[2]);
	const double l2 = dot3(d0, d1, d2, d0, d1, d2);
	const bool zero_i = n_i[0] == 0.f && n_i[1] == 0.f && n_i[2] == 0.f, zero_j = n_j[0] == 0.f && n_j[1] == 0.f && n_j[2] == 0.f;
	if (!(l2 > 0.0) || zero_i || zero_j) return false;
	const double l = root(l2);
	const double i0 = (double)n_i[0], i1 = (double)n_i[1], i2 = (double)n_i[2], j0 = (double)n_j[0], j1 = (double)n_j[1], j2 = (double)n_j[2];
	const double a1 = div(dot3(i0, i1, i2, d0, d1, d2), l), a2 = div(dot3(j0, j1, j2, d0, d1, d2), l);
	const bool swap = mag(a1) < mag(a2);
	const double s0 = swap ? j0 : i0, s1 = swap ? j1 : i1, s2 = swap ? j2 : i2, t0 = swap ? i0 : j0, t1 = swap ? i1 : j1, t2 = swap ? i2 : j2;
	const double f3 = swap ? -a2 : a1;
	if (swap) { d0 = -d0; d1 = -d1; d2 = -d2; }
	double v0 = sub(mul(d1, s2), mul(d2, s1)), v1 = sub(mul(d2, s0), mul(d0, s2)), v2 = sub(mul(d0, s1), mul(d1, s0));
	const double vl2 = dot3(v0, v1, v2, v0, v1, v2);
	if (!(vl2 > 0.0)) return false;
	const double vl = root(vl2);
	v0 = div(v0, vl); v1 = div(v1, vl); v2 = div(v2, vl);
	const double w0 = sub(mul(s1, v2), mul(s2, v1)), w1 = sub(mul(s2, v0), mul(s0, v2)), w2 = sub(mul(s0, v1), mul(s1, v0));
	const double f2 = dot3(v0, v1, v2, t0, t1, t2), x = dot3(s0, s1, s2, t0, t1, t2), y = dot3(w0, w1, w2, t0, t1, t2);
	b[0] = theta_bin(x, y);
	b[1] = bin11(f2);
	b[2] = bin11(f3);
	return true;
}
}  // namespace fpfh

// ---- RANSAC plane segmentation (kdbuild.hip; goicp_segment_plane_host / goicp_plane_filter_host are the host twins) ----
// What include/goicp_mi355.h defines per hypothesis and per pair, one text for the host path (kdtree.cpp) and the kernels: the counter-based
// draw (integers only), the plane of a triple (fp64, every operation rounded once, pca's + - * / sqrt), the sign rule and the float pair.
constexpr int kPlaneMaxIterations = 65536, kPlaneMaxPlanes = 8, kPlaneDefaultIterations = 1000;
constexpr int kPlaneWords = 16;   // the refit's integer moments: m, S_0..2, the high words of P_00 P_01 P_02 P_11 P_12 P_22, their low words
// goicp_plane_select with the defaults filled in (iterations and max_planes >= 1)
struct PlaneSelect {
	float distance = 0.f;
	int32_t iterations = 0, refine = 0, max_planes = 0, min_inliers = 0;
	uint64_t seed = 0;
};
struct PlaneRecord {                                           // goicp_plane, field for field
	float normal[3], point[3], d;
	int32_t inliers, hypothesis, refined;
};
namespace plane {
// h(c): the splitmix64 finaliser of seed + (c + 1) * 0x9E3779B97F4A7C15
GOICP_HD inline uint64_t hash(uint64_t seed, uint64_t c)
{
	uint64_t z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
// three distinct positions of a cloud of n >= 3 points for hypothesis number g = p * T + t
GOICP_HD inline void draw(uint64_t seed, uint64_t g, uint32_t n, uint32_t* a_out, uint32_t* b_out, uint32_t* c_out)
{
	const uint32_t a = (uint32_t)(hash(seed, 3ull * g) % (uint64_t)n);
	uint32_t b = (uint32_t)(hash(seed, 3ull * g + 1ull) % (uint64_t)(n - 1u));
	if (b >= a) b++;
	uint32_t c = (uint32_t)(hash(seed, 3ull * g + 2ull) % (uint64_t)(n - 2u));
	const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
	if (c >= lo) c++;
	if (c >= hi) c++;
	*a_out = a; *b_out = b; *c_out = c;
}
GOICP_HD inline bool finite3(const float v[3])
{
	// x - x is 0 for a finite x and NaN for an infinity or a NaN
	return v[0] - v[0] == 0.f && v[1] - v[1] == 0.f && v[2] - v[2] == 0.f;
}
// the normals operator's sign rule without a viewpoint: the first non-zero component positive, a zero written as +0
GOICP_HD inline void sign(float n[3])
{
	const float lead = n[0] != 0.f ? n[0] : (n[1] != 0.f ? n[1] : n[2]);
	const bool flip = lead < 0.f;
	for (int k = 0; k < 3; k++) n[k] = n[k] == 0.f ? 0.f : (flip ? -n[k] : n[k]);
}
// the float normal of the plane through pa, pb, pc; false: the hypothesis is degenerate (nrm is then not to be used)
GOICP_HD inline bool of_triple(const float* pa, const float* pb, const float* pc, float nrm[3])
{
	using namespace pca;
	const double u0 = sub((double)pb[0], (double)pa[0]), u1 = sub((double)pb[1], (double)pa[1]), u2 = sub((double)pb[2], (double)pa[2]);
	const double v0 = sub((double)pc[0], (double)pa[0]), v1 = sub((double)pc[1], (double)pa[1]), v2 = sub((double)pc[2], (double)pa[2]);
	const double n0 = sub(mul(u1, v2), mul(u2, v1)), n1 = sub(mul(u2, v0), mul(u0, v2)), n2 = sub(mul(u0, v1), mul(u1, v0));
	const double l2 = add(add(mul(n0, n0), mul(n1, n1)), mul(n2, n2));
	if (!(l2 > 0.0)) return false;
	const double len = root(l2);
	nrm[0] = (float)div(n0, len); nrm[1] = (float)div(n1, len); nrm[2] = (float)div(n2, len);
	if (!finite3(nrm)) return false;
	sign(nrm);
	return true;
}
// the pair: is the point within `distance` of the plane through a with normal n?  Float, left to right; a NaN compares false
GOICP_HD inline bool inlier(float x, float y, float z, float a0, float a1, float a2, float n0, float n1, float n2, float distance)
{
	const float e = ((x - a0) * n0 + (y - a1) * n1) + (z - a2) * n2;
	return (e < 0.f ? -e : e) <= distance;
}
// ax + by + cz + d = 0
GOICP_HD inline float offset(const float n[3], const float p[3])
{
	using namespace pca;
	return (float)-add(add(mul((double)n[0], (double)p[0]), mul((double)n[1], (double)p[1])), mul((double)n[2], (double)p[2]));
}
}  // namespace plane
// The refit's host finish, which both paths call on the 16 integer words (kdtree.cpp): the covariance from exact 128-bit integers, the
// normals operator's Jacobi, the smallest eigenvalue's column as the float normal, the centroid as the anchor.  mn / e: the frame of the
// round's cloud (E < 2^e).  false: no usable normal (the refit then does not stand)
bool plane_refit(const unsigned long long words[kPlaneWords], const float mn[3], int e, float normal[3], float point[3]);
// d_xyz: the n points on the device; s: the resolved selection.  d_label (may be null): n ints, -1 or the plane that took the point;
// d_out (may be null): room for 3 n floats, the first 3 * *m are the points no plane took, input order, own bits; d_index (may be null, only
// with d_out): their original indices.  planes: room for s.max_planes records on the host; *n_planes of them are written.  Between the rounds
// 8 bytes (the best key), the best hypothesis' 32 and the refit's 128 + 4 come back.  Returns after the stream has drained
hipError_t launch_segment_plane(const float* d_xyz, int n, const PlaneSelect& s, int32_t* d_label, float* d_out, int32_t* d_index, PlaneRecord* planes,
                                int* n_planes, int* m, hipStream_t stream, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);

// ---- RANSAC pose estimation from correspondences (kdbuild.hip; goicp_ransac_pose_host is the host twin) ----
// What include/goicp_mi355.h defines per hypothesis and per pair, one text for the host path (kdtree.cpp), the kernels and the refit's host
// finish: plane's draw, the edge-length pre-rejection and the rotation of a cross-covariance (fp64, every operation rounded once, pca's
// + - * / sqrt and its Jacobi), and the float pair.
constexpr int kRansacPoseMaxIterations = 1 << 20, kRansacPoseMaxPoses = 64, kRansacPoseDefaultIterations = 100000;
constexpr int kRansacPoseWords = 25;   // the refit's integer moments: m, Ss_0..2, St_0..2, the high words of the nine P_ab (3 a + b), their low words
constexpr int kRpBlock = 256;          // threads of a score workgroup: 4 waves
constexpr int kRpPts = 4;              // correspondences a lane keeps in registers: 1 024 per workgroup
constexpr int kRpTile = 256;           // hypotheses of a workgroup's LDS tile (12 KB of poses + 1 KB of counts)
// goicp_ransac_pose_select with the defaults filled in (iterations and max_poses >= 1)
struct RansacPoseSelect {
	float distance = 0.f;
	int32_t iterations = 0, refine = 0, max_poses = 0, min_inliers = 0;
	float edge_similarity = 0.f;
	uint64_t seed = 0;
};
struct RansacPoseRecord {                                      // goicp_ransac_pose, field for field
	float R[9], t[3];
	int32_t inliers, hypothesis, refined;
};
// the frame of one side of the correspondences (the voxel operator's: mn_k, E = max (x_k - mn_k) in float, E < 2^e by frexp)
struct RansacPoseFrame {
	float mn[3];
	int e;
};
namespace pose {
using pca::add; using pca::sub; using pca::mul; using pca::div; using pca::root;
using fpfh::dot3;
GOICP_HD inline double len2_of_edge(const float* p, const float* q)
{
	const double d0 = sub((double)q[0], (double)p[0]), d1 = sub((double)q[1], (double)p[1]), d2 = sub((double)q[2], (double)p[2]);
	return dot3(d0, d1, d2, d0, d1, d2);
}
// the pre-rejection of one edge: min(ls2, lt2) >= ss * max(ls2, lt2), ss = sigma * sigma in fp64
GOICP_HD inline bool edge_ok(const float* sp, const float* sq, const float* tp, const float* tq, double ss)
{
	const double ls2 = len2_of_edge(sp, sq), lt2 = len2_of_edge(tp, tq);
	const double lo = ls2 < lt2 ? ls2 : lt2, hi = ls2 < lt2 ? lt2 : ls2;
	return lo >= mul(ss, hi);
}
GOICP_HD inline bool triple_ok(const float* sa, const float* sb, const float* sc, const float* ta, const float* tb, const float* tc, float sigma)
{
	const double ss = mul((double)sigma, (double)sigma);
	return edge_ok(sa, sb, ta, tb, ss) && edge_ok(sb, sc, tb, tc, ss) && edge_ok(sc, sa, tc, ta, ss);
}
// swap the pair (l, column) i, j of the eigen-decomposition when l_j > l_i (selects on values: an index into V would put it into scratch)
#define GOICP_POSE_ORDER(li, lj, xi, yi, zi, xj, yj, zj) \
	do { \
		const bool sw = lj > li; \
		const double tl = sw ? lj : li, tx = sw ? xj : xi, ty = sw ? yj : yi, tz = sw ? zj : zi; \
		lj = sw ? li : lj; xj = sw ? xi : xj; yj = sw ? yi : yj; zj = sw ? zi : zj; \
		li = tl; xi = tx; yi = ty; zi = tz; \
	} while (0)
// The rotation and translation that take the source onto the target in the least-squares sense from the cross-covariance
// H_ab = sum (m_a - ct_a)(s_b - cs_b) (target rows, source columns; any positive scale) and the centroids cs, ct.  false: degenerate (R, t
// are then not to be used)
GOICP_HD inline bool from_cross_covariance(const double H[3][3], const double cs[3], const double ct[3], float R[9], float t[3])
{
	double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
	for (int a = 0; a < 3; a++)
		for (int b = 0; b < 3; b++) A[a][b] = dot3(H[0][a], H[1][a], H[2][a], H[0][b], H[1][b], H[2][b]);
	for (int sweep = 0; sweep < pca::kMaxSweeps; sweep++) {
		const bool r01 = pca::rotate<0, 1>(A, V), r02 = pca::rotate<0, 2>(A, V), r12 = pca::rotate<1, 2>(A, V);
		if (!(r01 || r02 || r12)) break;
	}
	// descending l, the lower index first on equal values: the three adjacent exchanges of a stable sort
	double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
	double x0 = V[0][0], y0 = V[1][0], z0 = V[2][0], x1 = V[0][1], y1 = V[1][1], z1 = V[2][1], x2 = V[0][2], y2 = V[1][2], z2 = V[2][2];
	GOICP_POSE_ORDER(l0, l1, x0, y0, z0, x1, y1, z1);
	GOICP_POSE_ORDER(l1, l2, x1, y1, z1, x2, y2, z2);
	GOICP_POSE_ORDER(l0, l1, x0, y0, z0, x1, y1, z1);
	if (!(l1 > 0.0)) return false;                               // rank below 2: collinear or coincident points
	double u0[3], u1[3];
	for (int a = 0; a < 3; a++) { u0[a] = dot3(H[a][0], H[a][1], H[a][2], x0, y0, z0); u1[a] = dot3(H[a][0], H[a][1], H[a][2], x1, y1, z1); }
	const double n0 = root(dot3(u0[0], u0[1], u0[2], u0[0], u0[1], u0[2])), n1 = root(dot3(u1[0], u1[1], u1[2], u1[0], u1[1], u1[2]));
	for (int a = 0; a < 3; a++) { u0[a] = div(u0[a], n0); u1[a] = div(u1[a], n1); }
	const double d = dot3(u0[0], u0[1], u0[2], u1[0], u1[1], u1[2]);
	for (int a = 0; a < 3; a++) u1[a] = sub(u1[a], mul(d, u0[a]));
	const double n2 = root(dot3(u1[0], u1[1], u1[2], u1[0], u1[1], u1[2]));
	for (int a = 0; a < 3; a++) u1[a] = div(u1[a], n2);
	const double u2[3] = {sub(mul(u0[1], u1[2]), mul(u0[2], u1[1])), sub(mul(u0[2], u1[0]), mul(u0[0], u1[2])), sub(mul(u0[0], u1[1]), mul(u0[1], u1[0]))};
	const double v0[3] = {x0, y0, z0}, v1[3] = {x1, y1, z1};
	const double v2[3] = {sub(mul(y0, z1), mul(z0, y1)), sub(mul(z0, x1), mul(x0, z1)), sub(mul(x0, y1), mul(y0, x1))};
	bool ok = true;
	for (int a = 0; a < 3; a++) {
		for (int b = 0; b < 3; b++) R[3 * a + b] = (float)add(add(mul(u0[a], v0[b]), mul(u1[a], v1[b])), mul(u2[a], v2[b]));
		t[a] = (float)sub(ct[a], dot3((double)R[3 * a], (double)R[3 * a + 1], (double)R[3 * a + 2], cs[0], cs[1], cs[2]));
		ok = ok && plane::finite3(R + 3 * a) && t[a] - t[a] == 0.f;
	}
	return ok;
}
#undef GOICP_POSE_ORDER
// the pose of three correspondences (source points sa, sb, sc onto target points ta, tb, tc); false: degenerate
GOICP_HD inline bool of_triple(const float* sa, const float* sb, const float* sc, const float* ta, const float* tb, const float* tc, float R[9], float t[3])
{
	double cs[3], ct[3], H[3][3];
	for (int k = 0; k < 3; k++) {
		cs[k] = div(add(add((double)sa[k], (double)sb[k]), (double)sc[k]), 3.0);
		ct[k] = div(add(add((double)ta[k], (double)tb[k]), (double)tc[k]), 3.0);
	}
	for (int a = 0; a < 3; a++)
		for (int b = 0; b < 3; b++)
			H[a][b] = add(add(mul(sub((double)ta[a], ct[a]), sub((double)sa[b], cs[b])), mul(sub((double)tb[a], ct[a]), sub((double)sb[b], cs[b]))),
			              mul(sub((double)tc[a], ct[a]), sub((double)sc[b], cs[b])));
	return from_cross_covariance(H, cs, ct, R, t);
}
// the pair: does the pose take the source point within sqrt(d2max) of the target point?  Float, left to right; a NaN compares false
// one axis of it: row (r0, r1, r2 | t) of the pose
GOICP_HD inline float residual(float r0, float r1, float r2, float t, float x0, float x1, float x2, float m) { return (((r0 * x0 + r1 * x1) + r2 * x2) + t) - m; }
GOICP_HD inline bool within(float e0, float e1, float e2, float d2max) { return (e0 * e0 + e1 * e1) + e2 * e2 <= d2max; }
GOICP_HD inline bool inlier(const float R[9], const float t[3], float x0, float x1, float x2, float m0, float m1, float m2, float d2max)
{
	return within(residual(R[0], R[1], R[2], t[0], x0, x1, x2, m0), residual(R[3], R[4], R[5], t[1], x0, x1, x2, m1),
	              residual(R[6], R[7], R[8], t[2], x0, x1, x2, m2), d2max);
}
}  // namespace pose
// The refit's host finish, which both paths call on the 25 integer words (kdtree.cpp): the cross-covariance from exact 128-bit integers, the
// centroids as the voxel operator forms them (kept in fp64), pose::from_cross_covariance.  false: no usable pose (the refit then does not stand)
bool ransac_pose_refit(const unsigned long long words[kRansacPoseWords], const RansacPoseFrame& fs, const RansacPoseFrame& ft, float R[9], float t[3]);
// d_src / d_tgt: the two clouds on the device, d_corr: M x 2 ints (source, target), every index in range; s: the resolved selection; fs / ft:
// the frames of the two sides (ransac_pose_frames, kdtree.cpp; read only with s.refine).  poses: room for s.max_poses records on the host,
// *n_poses of them are written; d_inlier (may be null): M bytes, the pair's verdict under pose 0, zeros without one.  8 + 48 bytes per
// returned pose and, with refine, 200 more come back.  Returns after the stream has drained
hipError_t launch_ransac_pose(const float* d_src, const float* d_tgt, const int32_t* d_corr, int M, const RansacPoseSelect& s, const RansacPoseFrame& fs,
                              const RansacPoseFrame& ft, RansacPoseRecord* poses, int* n_poses, unsigned char* d_inlier, hipStream_t stream,
                              hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);

// per-axis minimum and maximum of n points on the device (one rocPRIM reduction, 24 bytes come back): the frame of a cloud that a device
// stage produced and the host has not seen.  Returns after the stream has drained
hipError_t launch_cloud_minmax(const float* d_xyz, int n, float mn[3], float mx[3], hipStream_t stream);

// ---- distance transform build (DT3D::Build, jly_3ddt.cpp:889-979; exact EDT) -------------------
// work: V^3 int32 (linear).  out: V^3 floats in dt.layout (may alias work only for layout 0).
hipError_t launch_dt_build(const float* model_xyz, int M, const DtDesc& dt, int32_t* work, float* out,
                           hipStream_t stream);
hipError_t launch_dt_to_half(const float* bricked, void* out_half, size_t n, hipStream_t stream);
// nearest-target-point table: the same exact EDT passes, carrying the arg-min.  pts: the k-d tree's leaf slots (padding slots
// have infinite coordinates); work_d / work_id: V^3 int32 each (linear); out: ids in dt.layout (V^3, or VB^3 x 64 bricked)
hipError_t launch_nn_seed_build(const float4* pts, int nslots, const DtDesc& dt, int32_t* work_d, int32_t* work_id, int32_t* out, hipStream_t stream);

}  // namespace goicp
