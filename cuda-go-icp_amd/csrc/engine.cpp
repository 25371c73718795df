// Engine: resident data set-up, batched branch-and-bound driver, ICP loop.
//
// Search semantics = reference CPU Go-ICP (src/goicp/jly_goicp.cpp):
//   outer best-first BnB over the angle-axis cube [-pi,pi]^3 (OuterBnB, :342-567), nested
//   best-first BnB over the translation cube [-0.5,0.5]^3 (InnerBnB, :227-340), ICP refinement
//   whenever the upper bound improves (:495-530), stop when best - lb <= SSEThresh.
// What is MI355X-first here: the reference evaluates ONE cube per step; this driver keeps the same
// bounds and the same queues but expands `trans_batch` translation nodes of every active inner search
// per kernel launch, and `rot_batch` rotation nodes at once (their children's upper- and lower-bound
// searches run in lock-step): thousands of cube x point evaluations per launch instead of one pass
// over N points.  Any expansion order of a best-first BnB yields valid bounds; with trans_batch = 1
// and wide_children = 0 the visit order is exactly the reference's.
#include "engine.hpp"
#include "comm.hpp"
#include "trace.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>

namespace goicp {

namespace {

// constants spelled as the reference does (jly_goicp.h:35-36)
constexpr double kPI = 3.1415926536;
constexpr double kSQRT3 = 1.732050808;
constexpr int kMaxRotLevel = 20;

double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// adds the milliseconds its scope took to `acc`
struct ScopedMs {
	double& acc;
	double t0 = now_ms();
	~ScopedMs() { acc += now_ms() - t0; }
};

// a cloud of the host's on the device: the copy is queued on the stream
Buf<float> upload_cloud(const float* xyz, size_t n, hipStream_t stream)
{
	Buf<float> d(3 * n);
	HIPCHK(hipMemcpyAsync(d, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, stream));
	return d;
}

}  // namespace

Engine::DeviceGuard::DeviceGuard(int dev) : want(dev)
{
	if (hipGetDevice(&prev) != hipSuccess) prev = -1;
	if (prev != want) HIPCHK(hipSetDevice(want));
}
Engine::DeviceGuard::~DeviceGuard()
{
	if (prev >= 0 && prev != want) hipSetDevice(prev);
}

void* Engine::scratch_bytes(size_t bytes)
{
	if (bytes > d_opscratch_.size()) {
		HIPCHK(hipStreamSynchronize(stream_));
		d_opscratch_.alloc(std::max(bytes, (size_t)1 << 16));
	}
	return d_opscratch_.get();
}

struct Engine::InnerSearch {
	int rot_slot = 0;
	float coeff = 0.f;            // 0 => upper-bound pass (maxRotDisL == NULL)
	float best = 0.f;             // optErrorT
	Node best_node{};
	bool improved = false;
	bool done = false;
	std::priority_queue<Node> pq;
	std::vector<Node> parents;    // popped this round
	long long pops = 0, cubes = 0;
	float min_ub = std::numeric_limits<float>::infinity();   // smallest upper bound of any cube evaluated
	int stale = 0;                // rounds since the incumbent last improved (host fallback: round widening)
	void finish(const SearchOut& o) { best = o.best; improved = o.improved; best_node = o.best_node; pops = o.pops; cubes = o.cubes; min_ub = o.min_ub; done = true; }
};

Engine::SearchOut Engine::SearchOut::of(const InnerSearch& s) { return SearchOut{s.best, s.improved, s.best_node, s.pops, s.cubes, s.min_ub}; }
Engine::SearchOut Engine::SearchOut::of(const QSearch& q) { return SearchOut{q.best, q.improved != 0, Node{q.bx, q.by, q.bz, q.bw, 0.f, 0.f, 0}, q.pops, q.cubes, q.min_ub}; }

Engine::InnerSearch Engine::fresh_search(int rot_slot, float coeff, float incumbent) const
{
	InnerSearch s;
	s.rot_slot = rot_slot; s.coeff = coeff; s.best = incumbent;
	s.pq.push(trans_root_);
	return s;
}

float Engine::rot_coeff(int level) const
{
	if (level < 0) return 0.f;
	return rot_coeff_[level < kMaxRotLevel ? level : kMaxRotLevel - 1];
}

// init runs in a DELEGATING constructor: the object counts as constructed once the private constructor returns, so when init throws,
// ~Engine runs before the members go -- a half-built engine is released on its own device like a whole one
Engine::Engine(const Params& p, size_t M, size_t N) : p_(p), M_(M), N_(N) {}
Engine::Engine(const Params& p, const float* target, size_t M, const float* source, size_t N) : Engine(p, M, N)
{
	init(target, M, source, N);
}

void Engine::init(const float* target, size_t M, const float* source, size_t N)
{
	if (!target || !source || M == 0 || N == 0) throw std::invalid_argument("goicp: empty target or source cloud");
	if (M > (size_t)INT32_MAX / 8 || N > (size_t)INT32_MAX / 8) throw std::invalid_argument("goicp: cloud too large");
	if (p_.dt_size < 8 || p_.dt_size > 640) throw std::invalid_argument("goicp: dt_size must be in [8,640]");
	if (!(p_.dt_expand >= 1.0) || !(p_.dt_expand <= 64.0)) throw std::invalid_argument("goicp: dt_expand must be in [1,64]");
	if (!(p_.mse_threshold > 0.f)) p_.mse_threshold = 1e-10f;             // the reference clamps the same way (src/common.cpp:64)
	for (size_t i = 0; i < 3 * M; i++) if (!std::isfinite(target[i])) throw std::invalid_argument("goicp: non-finite coordinate in the target cloud");
	for (size_t i = 0; i < 3 * N; i++) if (!std::isfinite(source[i])) throw std::invalid_argument("goicp: non-finite coordinate in the source cloud");
	double t_mark = now_ms();
	TraceRange tr_create("goicp:create");
	static const char* const kStages[] = {"goicp:create:device_setup", "goicp:create:source_order_upload", "goicp:create:distance_transform",
	                                      "goicp:create:kd_hierarchy", "goicp:create:staging_buffers", "goicp:create:end"};
	int stage = 0;
	Trace::get().push(kStages[0]);
	struct PopLast { ~PopLast() { Trace::get().pop(); } } pop_last;     // the stage range open when init returns or throws
	auto lap = [&](const char* what) {
		if (p_.verbose) std::fprintf(stderr, "[goicp] create: %-28s %8.2f ms\n", what, now_ms() - t_mark);
		t_mark = now_ms();
		if (Trace::get().on()) { Trace::get().pop(); stage = std::min(stage + 1, 5); Trace::get().push(kStages[stage]); }
	};
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
		throw std::runtime_error("goicp: no HIP device available (this engine has no CPU fallback)");
	if (p_.device >= ndev) throw std::invalid_argument("goicp: device ordinal out of range");
	if (p_.device >= 0) dev_ = p_.device; else HIPCHK(hipGetDevice(&dev_));
	DeviceGuard guard(dev_);
	if (p_.stream_priority > 0) {
		int least = 0, greatest = 0;
		HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
		stream_.create(greatest);
	} else
		stream_.create();
	ev0_.create();
	ev1_.create();
	// lane 1's stream is made here, not in a timed registration (a stream costs ~2 ms to create); lanes 2.. make theirs on first use
	lane_stream_[0] = stream_;
	make_lane_stream(1);
	ev_fork_.create(hipEventDisableTiming);
	lanes_ = p_.lanes; lane_min_searches_ = std::max(2, p_.lane_min_searches);

	h_target_.assign(target, target + 3 * M);
	if (!(p_.trim_fraction >= 0.f) || p_.trim_fraction >= 1.f) throw std::invalid_argument("goicp: trim_fraction must be in [0,1)");
	icp_err_diff_ = p_.mse_threshold / 10000;        // jly_goicp.cpp:186

	// ---- search domain: the CPU path's roots (jly_goicp.cpp:44-53) unless the configured ranges narrow it ----
	rot_root_ = Node{(float)-kPI, (float)-kPI, (float)-kPI, (float)(2 * kPI), 0.f, 0.f, 0};
	trans_root_ = Node{-0.5f, -0.5f, -0.5f, 1.0f, 0.f, 0.f, 0};
	auto cube_of_box = [](const float lo[3], const float hi[3], Node* root) {
		float w = 0.f;
		for (int k = 0; k < 3; k++) {
			if (!(hi[k] >= lo[k]) || !std::isfinite(lo[k]) || !std::isfinite(hi[k])) throw std::invalid_argument("goicp: empty or non-finite search range");
			w = std::max(w, hi[k] - lo[k]);
		}
		if (!(w > 0.f)) w = 1e-6f;          // a point range: one tiny cube
		// An axis of zero width (rotation about one axis only, a fixed translation component): centred, its value would sit
		// exactly on the first split plane, and the strict in_box test would drop BOTH children -- the search would end
		// after one pop with the initial ICP pose.  Such an axis is placed a third of the way into the root instead: a
		// third is not a dyadic fraction, so the value is interior to exactly one cube at every level.
		float c[3];
		for (int k = 0; k < 3; k++) c[k] = hi[k] > lo[k] ? (lo[k] + hi[k]) / 2 - w / 2 : lo[k] - w / 3;
		root->x = c[0]; root->y = c[1]; root->z = c[2];
		root->w = w;
	};
	if (p_.use_rot_range) {
		bool full = true;
		for (int k = 0; k < 3; k++) full = full && p_.rot_min[k] <= -180.f && p_.rot_max[k] >= 180.f;
		if (!full) {
			for (int k = 0; k < 3; k++) {
				rot_lo_[k] = std::max((float)-kPI, (float)((double)p_.rot_min[k] * kPI / 180.0));
				rot_hi_[k] = std::min((float)kPI, (float)((double)p_.rot_max[k] * kPI / 180.0));
			}
			cube_of_box(rot_lo_, rot_hi_, &rot_root_);
			rot_boxed_ = true;
		}
	}
	if (p_.use_trans_range) {
		for (int k = 0; k < 3; k++) { trans_lo_[k] = p_.trans_min[k]; trans_hi_[k] = p_.trans_max[k]; }
		cube_of_box(trans_lo_, trans_hi_, &trans_root_);
		// a cubic range IS the root: nothing to cull
		trans_boxed_ = !(trans_hi_[0] - trans_lo_[0] == trans_root_.w && trans_hi_[1] - trans_lo_[1] == trans_root_.w && trans_hi_[2] - trans_lo_[2] == trans_root_.w);
	}

	// rotation uncertainty coefficients per level (jly_goicp.cpp:153-159); level l = cubes of width root/2^l
	for (int l = 0; l < kMaxRotLevel; l++) {
		float w0 = rot_root_.w;
		float sigma = (float)((double)w0 / std::pow(2.0, l) / 2.0);
		float maxAngle = (float)(kSQRT3 * (double)sigma);
		if ((double)maxAngle > kPI) maxAngle = (float)kPI;
		rot_coeff_[l] = 2 * std::sin(maxAngle / 2);
	}

	lap("validation + device setup");
	// ---- source cloud: (x,y,z,|p|), ordered for gather locality (morton_sort: 0 input order, 1 Morton curve, 2 k-d order) ----
	load_source(source, N, false);

	lap("source order + upload");
	// ---- distance transform geometry (jly_3ddt.cpp:891-923), double ----
	{
		double xMin = target[0], xMax = target[0], yMin = target[1], yMax = target[1], zMin = target[2], zMax = target[2];
		double cm[3] = {0, 0, 0};
		for (size_t i = 0; i < M_; i++) {
			double x = target[3 * i], y = target[3 * i + 1], z = target[3 * i + 2];
			if (xMin > x) xMin = x;
			if (xMax < x) xMax = x;
			if (yMin > y) yMin = y;
			if (yMax < y) yMax = y;
			if (zMin > z) zMin = z;
			if (zMax < z) zMax = z;
			cm[0] += x; cm[1] += y; cm[2] += z;
		}
		for (int k = 0; k < 3; k++) model_centroid_[k] = (float)(cm[k] / (double)M_);
		const double ex = p_.dt_expand;
		double xc = (xMin + xMax) / 2, yc = (yMin + yMax) / 2, zc = (zMin + zMax) / 2;
		xMin = xc - ex * (xMax - xc); xMax = xc + ex * (xMax - xc);
		yMin = yc - ex * (yMax - yc); yMax = yc + ex * (yMax - yc);
		zMin = zc - ex * (zMax - zc); zMax = zc + ex * (zMax - zc);
		double side = xMax - xMin > yMax - yMin ? xMax - xMin : yMax - yMin;
		side = side > zMax - zMin ? side : zMax - zMin;
		if (!(side > 0)) throw std::invalid_argument("goicp: degenerate target cloud (zero extent)");
		dt_.V = p_.dt_size;
		dt_.VB = (p_.dt_size + 3) / 4;
		dt_.layout = p_.dt_layout ? 1 : 0;
		dt_.xmin = xc - side / 2; dt_.ymin = yc - side / 2; dt_.zmin = zc - side / 2;
		dt_.scale = dt_.V / side;
		dt_.scale_f = (float)dt_.scale; dt_.xmin_f = (float)dt_.xmin; dt_.ymin_f = (float)dt_.ymin; dt_.zmin_f = (float)dt_.zmin;
		// float index fast path: 2^-24 * (scale*|min| + 3|F| + 2) bounds the rounding of min_f, scale_f,
		// (q - min_f) and the fma; shipped with a margin (4|F| + 8, x1.05)
		const double s0 = dt_.scale * std::max({std::fabs(dt_.xmin), std::fabs(dt_.ymin), std::fabs(dt_.zmin)});
		dt_.c1 = (float)(1.05 * std::ldexp(1.0, -24) * (s0 + 8.0));
		dt_.c2 = (float)(1.05 * std::ldexp(1.0, -24) * 4.0);
	}
	update_bounds_cost();                     // reads the geometry only: it runs beside the DT build
	// ---- DT build on the GPU ----
	{
		double t0 = now_ms();
		const size_t V = dt_.V, nlin = V * V * V;
		const size_t nout = dt_.layout ? (size_t)dt_.VB * dt_.VB * dt_.VB * 64 : nlin;
		Buf<float> model_buf(3 * M_);
		Buf<int32_t> work_buf;
		float* d_model = model_buf;
		d_dt_.alloc(nout);
		if (dt_.layout) {
			work_buf.alloc(nlin);
			HIPCHK(hipMemsetAsync(d_dt_, 0, sizeof(float) * nout, stream_));
		}
		int32_t* d_work = dt_.layout ? work_buf.get() : reinterpret_cast<int32_t*>(d_dt_.get());   // the linear grid is built in place
		HIPCHK(hipMemcpyAsync(d_model, target, sizeof(float) * 3 * M_, hipMemcpyHostToDevice, stream_));
		dt_.grid = d_dt_;
		{   // table of the out-of-grid extension term, same float sqrt + double divide as the kernel's fallback
			const int n = 16384;
			std::vector<double> tab(n);
			for (int i = 0; i < n; i++) tab[i] = (double)std::sqrt((float)i) / dt_.scale;
			d_overshoot_.alloc(n);
			HIPCHK(hipMemcpyAsync(d_overshoot_, tab.data(), sizeof(double) * n, hipMemcpyHostToDevice, stream_));
			HIPCHK(hipStreamSynchronize(stream_));
			dt_.overshoot = d_overshoot_; dt_.n_overshoot = n;
		}
		HIPCHK(launch_dt_build(d_model, (int)M_, dt_, d_work, d_dt_, stream_));
		if (p_.bounds_fp16 && dt_.layout == 1) {
			d_dt16_.alloc(nout);
			HIPCHK(launch_dt_to_half(d_dt_, d_dt16_, nout, stream_));
			dt16_ = dt_;
			dt16_.grid = reinterpret_cast<const float*>(d_dt16_.get());
			dt16_.layout = 2;
		}
		HIPCHK(hipStreamSynchronize(stream_));
		dt_build_ms_ = now_ms() - t0;
	}
	lap("distance transform");
	// ---- k-d tree (64-ary box hierarchy) over the target ----
	{
		// auto = host median splits: at 1 M points the device (Morton) build is 0.3 s quicker to make, but its
		// looser boxes double every ICP pass (3.2 vs 1.65 ms) -- 0.56 s over one registration
		const bool gpu_build = p_.kd_gpu_build > 0;
		if (!gpu_build) {
			KdHost kh;
			build_kdtree(target, (int)M_, kLeafSlots, &kh);
			for (int l = 0; l < kh.K; l++) {
				d_kd_boxes_[l].alloc(kh.boxes[l].size());
				HIPCHK(hipMemcpy(d_kd_boxes_[l], kh.boxes[l].data(), sizeof(float) * kh.boxes[l].size(), hipMemcpyHostToDevice));
			}
			d_kd_pts_.alloc(kh.pts.size());
			HIPCHK(hipMemcpy(d_kd_pts_, kh.pts.data(), sizeof(float4) * kh.pts.size(), hipMemcpyHostToDevice));
			kd_.K = kh.K;
			kd_slots_ = kh.pts.size();
		} else {
			// device build: Morton sort + bottom-up boxes, no host tree
			int K = 1;
			while (K < kMaxLevels && (long long)kLeafSlots * (1LL << (6 * K)) < (long long)M_) K++;
			if ((long long)kLeafSlots * (1LL << (6 * K)) < (long long)M_) throw std::invalid_argument("goicp: target cloud too large for the k-d tree");
			Buf<float> model_buf(3 * M_);
			float* d_model = model_buf;
			HIPCHK(hipMemcpyAsync(d_model, target, sizeof(float) * 3 * M_, hipMemcpyHostToDevice, stream_));
			for (int l = 0; l < K; l++) d_kd_boxes_[l].alloc(384 * ((size_t)1 << (6 * l)));
			d_kd_pts_.alloc(kLeafSlots * ((size_t)1 << (6 * K)));
			float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
			for (size_t i = 0; i < M_; i++)
				for (int k = 0; k < 3; k++) { mn[k] = std::min(mn[k], target[3 * i + k]); mx[k] = std::max(mx[k], target[3 * i + k]); }
			const float ext = std::max({mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]});
			float* boxes[kMaxLevels];
			for (int l = 0; l < kMaxLevels; l++) boxes[l] = d_kd_boxes_[l];
			HIPCHK(launch_kd_build(d_model, (int)M_, K, mn, ext, boxes, d_kd_pts_, stream_));
			kd_.K = K;
			kd_slots_ = (size_t)kLeafSlots * ((size_t)1 << (6 * K));
		}
		for (int l = 0; l < kMaxLevels; l++) kd_.boxes[l] = d_kd_boxes_[l];
		kd_.pts = d_kd_pts_; kd_.M = (int)M_;
	}
	lap("k-d hierarchy + upload");
	if (p_.icp_point_seed) {
		// nearest-target-point table: per voxel the leaf slot of a target point whose seed voxel is nearest (the exact EDT passes
		// again, carrying their arg-min) -- the neighbour search of the ICP starts from that point instead of from a bound
		const size_t V = dt_.V, nlin = V * V * V;
		const size_t nout = dt_.layout ? (size_t)dt_.VB * dt_.VB * dt_.VB * 64 : nlin;
		const int nslots = (int)kd_slots_;                  // the slots that exist (the root group of the hierarchy is sparse: 16 x 2^D, not 16 x 64^K)
		Buf<int32_t> wd(nlin), wi(nlin);
		d_nn_ids_.alloc(nout);
		HIPCHK(hipMemsetAsync(d_nn_ids_, 0, sizeof(int32_t) * nout, stream_));          // brick padding beyond V: slot 0, never addressed
		HIPCHK(launch_nn_seed_build(d_kd_pts_, nslots, dt_, wd, wi, d_nn_ids_, stream_));
		HIPCHK(hipStreamSynchronize(stream_));
		dt_.nn_ids = d_nn_ids_;
		lap("nearest-point table");
	}
	d_icp_state_.alloc(1);
	d_icp_acc_.alloc((size_t)kIcpAccReplicas * kIcpAcc);
	HIPCHK(hipMemsetAsync(d_icp_acc_, 0, sizeof(unsigned long long) * kIcpAccReplicas * kIcpAcc, stream_));
	for (size_t i = 0; i < 3 * M_; i++) target_abs_max_ = std::max(target_abs_max_, std::fabs(target[i]));
	d_icp_ticket_.alloc(64 / sizeof(int));
	HIPCHK(hipMemset(d_icp_ticket_, 0, 64));
	h_icp_state_.alloc(3);      // [0] the state as uploaded / as last fetched, [1], [2] icp_run's two fetch slots
	ensure_batch(4096, 64);
	if (p_.device_queues && p_.trans_batch > 1 && p_.wide_children) {
		// the device-resident inner-BnB queues, sized for a full round of the outer search, and their pinned mirror touched
		// once (the first use of a fresh pinned block costs milliseconds -- measured 8 ms inside the first registration)
		ensure_lane(0, flow_mode() ? kFlowSearches : 1);
		if (flow_mode()) {
			ensure_batch(1, kFlowSearches / 2);
			h_qinit_.alloc(kFlowSearches);
			d_qinit_.alloc(kFlowSearches);
			std::memset(h_qinit_, 0, sizeof(QInit) * kFlowSearches);
		}
		std::memset(ql_[0].h_search, 0, sizeof(QSearch) * ql_[0].cap);
		HIPCHK(hipMemcpyAsync(ql_[0].d_search, ql_[0].h_search, sizeof(QSearch) * ql_[0].cap, hipMemcpyHostToDevice, stream_));
		HIPCHK(hipMemcpyAsync(ql_[0].h_search, ql_[0].d_search, sizeof(QSearch) * ql_[0].cap, hipMemcpyDeviceToHost, stream_));
		HIPCHK(hipMemcpyAsync(ql_[0].h_ctl, ql_[0].d_ctl, sizeof(QCtl), hipMemcpyDeviceToHost, stream_));
		HIPCHK(hipStreamSynchronize(stream_));
		// ... and one dummy search that stops at its root (incumbent 0): the first launch of each queue kernel loads its
		// code object, which belongs to engine creation, not to the first registration
		InnerSearch warm;
		warm.best = 0.f;
		std::vector<InnerSearch*> one{&warm};
		std::vector<Rot9> rot(1);
		const float I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
		std::memcpy(rot[0].r, I9, sizeof(I9));
		run_inner_device(one, rot);
		{
			// ... and the read-back of a batch's search records at the sizes a registration uses (tens of KB): measured on MI355X, the FIRST
			// device-to-host copy of such a size after kernels have run costs 8.6 ms (a one-time set-up inside the runtime; the 80-byte
			// read-back of the dummy search above does not trigger it, neither does the copy made before any kernel ran) -- it belongs to
			// engine creation, not to the first registration (full bunny: first run 43 -> 34 ms)
			const double tw = now_ms();
			for (size_t n = 1; n <= ql_[0].cap; n *= 2) HIPCHK(hipMemcpyAsync(ql_[0].h_search, ql_[0].d_search, sizeof(QSearch) * n, hipMemcpyDeviceToHost, stream_));
			HIPCHK(hipStreamSynchronize(stream_));
			if (p_.verbose) std::fprintf(stderr, "[goicp] create: read-back warm-up %.2f ms\n", now_ms() - tw);
		}
		if (flow_mode()) {
			// the same for the continuous-flow driver: its list-init kernel, the full-size rotation table upload and the
			// full-size read-back of the search records, once, here
			const QParams qp = queue_params();
			flow_reset();
			h_qinit_[0] = QInit{0, 0.f, 0.f, 0, -1};
			std::memcpy(h_rots_[0].r, I9, sizeof(I9));
			HIPCHK(hipMemcpyAsync(d_rots_, h_rots_, sizeof(Rot9) * (kFlowSearches / 2), hipMemcpyHostToDevice, stream_));
			HIPCHK(hipMemcpyAsync(d_qinit_, h_qinit_, sizeof(QInit) * kFlowSearches, hipMemcpyHostToDevice, stream_));
			HIPCHK(launch_bnb_init_list(ql_[0].d_search, ql_[0].d_nodes, d_qinit_, 1, qp, stream_));
			RoundOpts warm_round;
			warm_round.count = false;
			for (int r = 0; r < 3; r++, q_parity_ ^= 1) queue_round(ql_[0], kFlowSearches, qp, q_parity_, kFlowSearches * qp.K, warm_round);
			HIPCHK(hipMemcpyAsync(ql_[0].h_ctl, ql_[0].d_ctl, sizeof(QCtl), hipMemcpyDeviceToHost, stream_));
			HIPCHK(hipMemcpyAsync(ql_[0].h_search, ql_[0].d_search, sizeof(QSearch) * kFlowSearches, hipMemcpyDeviceToHost, stream_));
			HIPCHK(hipStreamSynchronize(stream_));
			flow_reset();
			HIPCHK(hipStreamSynchronize(stream_));
		}
		cnt_ = Counters{};
		queue_rounds_ = 0;
	}

	{
		// the first launch of the ICP kernels, of the scoring launch and their first state / result read-backs also belong to engine creation
		// (measured: the first registration's ICP stretch 18.3 ms against 13.2 ms for every later one)
		const double tw = now_ms();
		const float I0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z0[3] = {0, 0, 0};
		float Rw[9], tw3[3];
		std::memcpy(Rw, I0, sizeof(I0)); std::memcpy(tw3, Z0, sizeof(Z0));
		int itw = 0;
		icp_run(Rw, tw3, 2 * std::max(1, p_.icp_chunk) + 1, -1e30f, &itw);       // three chunks: both fetch slots and both events are used once
		(void)eval_sse(I0, Z0);
		cnt_ = Counters{};
		if (p_.verbose) std::fprintf(stderr, "[goicp] create: ICP + scoring warm-up %.2f ms\n", now_ms() - tw);
	}
	const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	std::memcpy(optR_, I, sizeof(I)); std::memcpy(curR_, I, sizeof(I)); std::memcpy(stepR_, I, sizeof(I));
	std::memset(optT_, 0, sizeof(optT_)); std::memset(curT_, 0, sizeof(curT_)); std::memset(stepT_, 0, sizeof(stepT_));
	publish(false);
	lap("staging buffers");
}

void Engine::check_source(const float* source, size_t N)
{
	if (!source || N == 0) throw std::invalid_argument("goicp: empty source cloud");
	if (N > (size_t)INT32_MAX / 8) throw std::invalid_argument("goicp: cloud too large");
	for (size_t i = 0; i < 3 * N; i++) if (!std::isfinite(source[i])) throw std::invalid_argument("goicp: non-finite coordinate in the source cloud");
}

void Engine::load_source(const float* source, size_t N, bool device_order, const float* d_xyz_ready)
{
	N_ = N;
	inliers_ = (int)((float)N_ * (1 - p_.trim_fraction));    // jly_goicp.cpp:201
	if (inliers_ < 1) inliers_ = 1;
	sse_thresh_ = p_.mse_threshold * (float)inliers_;         // jly_goicp.cpp:208
	d_src_.reserve(N_);
	std::vector<int32_t> perm(N_);
	const bool on_device = device_order && p_.morton_sort >= 1;
	Buf<float> d_up;          // what a device-ordered swap leaves on the device: the source normals below read both
	Buf<int32_t> d_perm;
	const float* d_xyz = nullptr;
	if (on_device) {
		// the order on the device (launch_source_order), the gather with |p| straight into d_src_; the permutation comes back for the
		// host mirror, whose sums below keep init's order of additions
		const int mode = p_.morton_sort == 1 ? 1 : 2;
		float mn[3] = {0, 0, 0}, ext = 1.f;
		if (mode == 1) source_morton_frame(source, N_, mn, &ext);
		d_up.alloc(d_xyz_ready ? 0 : 3 * N_);
		d_perm.alloc(N_);
		if (!d_xyz_ready) HIPCHK(hipMemcpyAsync(d_up, source, sizeof(float) * 3 * N_, hipMemcpyHostToDevice, stream_));
		d_xyz = d_xyz_ready ? d_xyz_ready : d_up.get();
		HIPCHK(hipEventRecord(ev0_, stream_));
		HIPCHK(launch_source_order(d_xyz, (int)N_, mode, mn, ext, d_perm, stream_));
		HIPCHK(hipEventRecord(ev1_, stream_));
		HIPCHK(launch_source_gather(d_xyz, d_perm, (int)N_, d_src_, stream_));
		HIPCHK(hipMemcpyAsync(perm.data(), d_perm, sizeof(int32_t) * N_, hipMemcpyDeviceToHost, stream_));
		HIPCHK(hipStreamSynchronize(stream_));
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		source_order_ms_ = ms;
	} else {
		source_order_host(source, N_, p_.morton_sort, perm.data());
	}
	src_perm_ = perm;
	h_src_sorted_.resize(4 * N_);
	double cs[3] = {0, 0, 0};
	for (size_t i = 0; i < N_; i++) {
		const float* s = source + 3 * (size_t)perm[i];
		float x = s[0], y = s[1], z = s[2];
		h_src_sorted_[4 * i] = x; h_src_sorted_[4 * i + 1] = y; h_src_sorted_[4 * i + 2] = z;
		h_src_sorted_[4 * i + 3] = std::sqrt(x * x + y * y + z * z);   // normData, jly_goicp.cpp:145
		cs[0] += x; cs[1] += y; cs[2] += z;
	}
	for (int k = 0; k < 3; k++) src_centroid_[k] = (float)(cs[k] / (double)N_);
	if (!on_device) HIPCHK(hipMemcpy(d_src_, h_src_sorted_.data(), sizeof(float4) * N_, hipMemcpyHostToDevice));
	src_radius_ = 0.f;
	for (size_t i = 0; i < N_; i++) src_radius_ = std::max(src_radius_, h_src_sorted_[4 * i + 3]);
	src_crad_ = -1.0;
	// ---- the N-sized buffers (grow-only: a smaller cloud uses the front of what is there, every kernel is bounded by N) ----
	const size_t partials = std::max(icp_partials_floats((int)N_), (size_t)icp_trim_blocks((int)N_) * kIcpAcc);
	d_icp_partials_.reserve(partials);
	if (inliers_ < (int)N_) { d_nn_d2_.reserve(N_); d_nn_slot_.reserve(N_); d_include_.reserve(N_); }
	if (p_.icp_nn_cache) {
		d_nn_cache_.reserve(2 * N_);
		HIPCHK(hipMemsetAsync(d_nn_cache_, 0, sizeof(float4) * 2 * N_, stream_));      // sqrt(best2_ref) = 0: the first pass walks
	}
	// the source normals, estimated or the caller's, belong to the cloud that just left; with the symmetric metric active the new cloud's are
	// part of the source stage (the first ICP after a swap is not charged for them), otherwise they are built on first use
	src_normals_k_ = 0;
	src_normals_user_ = false;
	if (source_normals_active()) build_source_normals(source, d_xyz, on_device ? d_perm.get() : nullptr);
	if (dt_.V > 0) update_bounds_cost();      // a swap; init counts once the grid's geometry is known
}

// what each of the source's eight chunks costs the pair launch (BoundsOrder::cost): one small launch behind the ordered source on the engine's
// stream, no wait of its own (init and every swap wait for the stream before they return)
void Engine::update_bounds_cost()
{
	if (!d_bcost_) d_bcost_.alloc(kBoundsCost + kBoundsPlan);
	const float a = p_.bounds_balance_a > 0.f ? p_.bounds_balance_a : kBoundsBalanceA;
	HIPCHK(launch_bounds_chunk_cost(d_src_, (int)N_, dt_, (int)std::min(a * 256.f + 0.5f, 16777216.f), d_bcost_, stream_));
}

void Engine::check_swap_size(size_t n, const char* fn) const
{
	if (reads_source_normals() && n < (size_t)source_normal_k_)
		throw std::invalid_argument(std::string(fn) + ": the cloud has fewer points than the handle's source_normal_k (goicp_set_icp_symmetric / goicp_set_icp_generalized)");
}

void Engine::sync_lane_streams()
{
	for (int k = 0; k < kMaxLanes; k++) if (lane_stream_[k]) HIPCHK(hipStreamSynchronize(lane_stream_[k]));   // lane 0 is the engine's stream
}

void Engine::set_source(const float* source, size_t N, const char* fn)
{
	// everything that can refuse comes first: a refused call leaves the engine as it was
	check_source(source, N);
	if (registering_.load()) throw std::invalid_argument(std::string(fn) + ": not while a registration runs");
	check_swap_size(N, fn);
	DeviceGuard guard(dev_);
	const double t0 = now_ms();
	TraceRange tr(fn);
	sync_lane_streams();
	load_source(source, N, true);
	finish_source_swap();
	if (p_.verbose) std::fprintf(stderr, "[goicp] %s: %zu points, %.2f ms (device order %.3f ms)\n", fn + 6, N_, now_ms() - t0, source_order_ms_);
}

void Engine::finish_source_swap()
{
	for (QLane& L : ql_) if (L.cap) lane_source_buffers(L);
	ensure_batch(4096, 64);                          // the bounds scratch depends on N
	// ---- the search and ICP state of a fresh engine; params, options, normals, callback, shard and the shard statistics stay ----
	cancel_.store(false);
	early_exit_ = converged_ = false;
	rot_ramp_ = 8;
	unrefined_ = false;
	last_round_work_ = 0; tile_sticky_ = false;
	icp_cache_active_ = false;
	while (!queue_.empty()) queue_.pop();
	if (flow_mode() && ql_[0].cap) flow_reset();
	cnt_ = Counters{};
	queue_rounds_ = 0; queue_fallbacks_ = 0; tile_rounds_ = 0;
	std::memset(sel_hist_, 0, sizeof(sel_hist_));
	std::memset(level_hist_, 0, sizeof(level_hist_));
	last_inliers_.clear(); last_robust_cost_.clear(); last_robust_w_.clear();   // no ICP has run on this cloud
	opt_err_ = 1e10f;
	register_ms_ = bnb_ms_ = icp_ms_ = 0;
	const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	std::memcpy(optR_, I, sizeof(I)); std::memcpy(curR_, I, sizeof(I)); std::memcpy(stepR_, I, sizeof(I));
	std::memset(optT_, 0, sizeof(optT_)); std::memset(curT_, 0, sizeof(curT_)); std::memset(stepT_, 0, sizeof(stepT_));
	HIPCHK(hipStreamSynchronize(stream_));
	{
		// the snapshot of a fresh engine (init publishes before a callback can be set: none is called here either)
		std::lock_guard<std::mutex> lk(mtx_);
		std::memcpy(snap_.optR, optR_, sizeof(optR_)); std::memcpy(snap_.optT, optT_, sizeof(optT_));
		std::memcpy(snap_.curR, curR_, sizeof(curR_)); std::memcpy(snap_.curT, curT_, sizeof(curT_));
		snap_.best_sse = opt_err_;
		snap_.finished = 0;
		snap_.counters = cnt_;
		snap_.dt_build_ms = dt_build_ms_;
		snap_.register_ms = register_ms_;
	}
}

void Engine::voxel_downsample(const float* xyz, size_t n, float voxel, float* out_xyz, int32_t* out_count, size_t* m_out)
{
	if (!out_xyz || !m_out) throw std::invalid_argument("goicp_voxel_downsample: out_xyz and m must be non-null");
	VoxelFrame f;
	voxel_frame(xyz, n, voxel, &f);
	if (registering_.load()) throw std::invalid_argument("goicp_voxel_downsample: not while a registration runs");
	DeviceGuard guard(dev_);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_), d_out(3 * n);
	Buf<int32_t> d_cnt(out_count ? n : 0);
	int m = 0;
	HIPCHK(launch_voxel_downsample(d_xyz, (int)n, f, d_out, out_count ? d_cnt.get() : nullptr, &m, stream_));
	HIPCHK(hipMemcpyAsync(out_xyz, d_out, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, stream_));
	if (out_count) HIPCHK(hipMemcpyAsync(out_count, d_cnt, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	*m_out = (size_t)m;
	if (p_.verbose) std::fprintf(stderr, "[goicp] voxel_downsample: %zu -> %d points\n", n, m);
}

void Engine::radius_outlier_removal(const float* xyz, size_t n, float radius, int32_t min_neighbors, float* out_xyz, int32_t* out_index,
                                    int32_t* out_count, size_t* m_out)
{
	if (!out_xyz || !m_out) throw std::invalid_argument("goicp_radius_outlier_removal: out_xyz and m must be non-null");
	VoxelFrame f;
	radius_frame(xyz, n, radius, min_neighbors, &f);
	if (registering_.load()) throw std::invalid_argument("goicp_radius_outlier_removal: not while a registration runs");
	DeviceGuard guard(dev_);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_), d_out(3 * n);
	Buf<int32_t> d_idx(out_index ? n : 0), d_cnt(out_count ? n : 0);
	int m = 0;
	HIPCHK(launch_radius_outlier_removal(d_xyz, (int)n, f, radius * radius, min_neighbors, d_out, out_index ? d_idx.get() : nullptr,
	                                     out_count ? d_cnt.get() : nullptr, &m, stream_));
	if (m > 0) HIPCHK(hipMemcpyAsync(out_xyz, d_out, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, stream_));
	if (out_index && m > 0) HIPCHK(hipMemcpyAsync(out_index, d_idx, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream_));
	if (out_count) HIPCHK(hipMemcpyAsync(out_count, d_cnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	*m_out = (size_t)m;
	if (p_.verbose) std::fprintf(stderr, "[goicp] radius_outlier_removal: %zu -> %d points\n", n, m);
}

namespace {

std::vector<float> stat_sample_host(const float* xyz, size_t n)
{
	const size_t ns = stat_sample_size(n), stride = n / ns;
	std::vector<float> s(3 * ns);
	for (size_t i = 0; i < ns; i++) std::memcpy(&s[3 * i], xyz + 3 * i * stride, 3 * sizeof(float));
	return s;
}

// the level plan of a cloud with these bounds: the frames and squared radii launch_stat_outlier_removal searches by
struct StatPlan {
	std::vector<VoxelFrame> frames;
	std::vector<float> r2;
	// sample: stat_sample_size(n) points, every (n / that)-th of the cloud
	StatPlan(const float mn[3], const float mx[3], size_t n, int32_t k, const std::vector<float>& sample)
	{
		float r = 0.f;
		int levels = 0;
		stat_levels(mn, mx, n, k, sample.data(), sample.size() / 3, &r, &levels);
		levels = std::min(levels, kStatMaxLevels);
		frames.resize((size_t)levels);
		r2.resize((size_t)levels);
		for (int L = 0; L < levels; L++, r *= 2.f) {
			radius_frame_of_box(mn, mx, n, r, 1, &frames[(size_t)L]);
			r2[(size_t)L] = r * r;
		}
	}
	// of a cloud the host holds, which stat_check_cloud checks on the way
	static StatPlan of_host_cloud(const float* xyz, size_t n, int32_t k)
	{
		float mn[3], mx[3];
		stat_check_cloud(xyz, n, mn, mx);
		return StatPlan(mn, mx, n, k, stat_sample_host(xyz, n));
	}
};

void stat_report_line(const char* what, size_t n, int m, const StatReport& rep)
{
	std::fprintf(stderr, "[goicp] %s: %zu -> %d points, levels %d, resolved", what, n, m, rep.levels_run + (rep.top > 0 ? 1 : 0));
	for (int L = 0; L < rep.levels_run; L++) std::fprintf(stderr, " %d", rep.resolved[L]);
	std::fprintf(stderr, ", top %d\n", rep.top);
}

}  // namespace

void Engine::statistical_outlier_removal(const float* xyz, size_t n, int32_t neighbors, float std_ratio, float* out_xyz, int32_t* out_index,
                                         float* out_mean_dist, double* threshold, size_t* m_out)
{
	if (!out_xyz || !m_out) throw std::invalid_argument("goicp_statistical_outlier_removal: out_xyz and m must be non-null");
	stat_check_params(n, neighbors, std_ratio);
	const StatPlan plan = StatPlan::of_host_cloud(xyz, n, neighbors);
	if (registering_.load()) throw std::invalid_argument("goicp_statistical_outlier_removal: not while a registration runs");
	DeviceGuard guard(dev_);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_), d_out(3 * n), d_mean(out_mean_dist ? n : 0);
	Buf<int32_t> d_idx(out_index ? n : 0);
	int m = 0;
	double thr = 0.0;
	StatReport rep;
	HIPCHK(launch_stat_outlier_removal(d_xyz, (int)n, plan.frames.data(), plan.r2.data(), (int)plan.frames.size(), neighbors, std_ratio, d_out,
	                                   out_index ? d_idx.get() : nullptr, out_mean_dist ? d_mean.get() : nullptr, &thr, &m, &rep, stream_));
	HIPCHK(hipMemcpyAsync(out_xyz, d_out, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, stream_));
	if (out_index) HIPCHK(hipMemcpyAsync(out_index, d_idx, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream_));
	if (out_mean_dist) HIPCHK(hipMemcpyAsync(out_mean_dist, d_mean, sizeof(float) * n, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	if (threshold) *threshold = thr;
	*m_out = (size_t)m;
	if (p_.verbose) stat_report_line("statistical_outlier_removal", n, m, rep);
}

void Engine::knn_self(const float* xyz, size_t n, int32_t k, int32_t* out_index, float* out_dist_sq)
{
	if (!out_index) throw std::invalid_argument("goicp_knn_self: out_index must be non-null");
	knn_self_check_params(n, k);
	const StatPlan plan = StatPlan::of_host_cloud(xyz, n, k);
	if (registering_.load()) throw std::invalid_argument("goicp_knn_self: not while a registration runs");
	DeviceGuard guard(dev_);
	const size_t rows = n * (size_t)k;
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_), d_d2(out_dist_sq ? rows : 0);
	Buf<int32_t> d_idx(rows);
	StatReport rep;
	HIPCHK(launch_self_knn(d_xyz, (int)n, plan.frames.data(), plan.r2.data(), (int)plan.frames.size(), k, d_idx, out_dist_sq ? d_d2.get() : nullptr, nullptr,
	                       &rep, stream_, ev0_, ev1_));
	HIPCHK(hipMemcpyAsync(out_index, d_idx, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, stream_));
	if (out_dist_sq) HIPCHK(hipMemcpyAsync(out_dist_sq, d_d2, sizeof(float) * rows, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	if (p_.verbose) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		stat_report_line("knn_self", n, (int)n, rep);
		std::fprintf(stderr, "[goicp] knn_self: k %d, device %.3f ms\n", k, ms);
	}
}

void Engine::estimate_normals(const float* xyz, size_t n, int32_t k, const float* vp, float* out_normals, float* out_variation, int32_t* out_index)
{
	if (!out_normals) throw std::invalid_argument("goicp_estimate_normals: out_normals must be non-null");
	normals_check_params(n, k, vp);
	const StatPlan plan = StatPlan::of_host_cloud(xyz, n, k - 1);
	if (registering_.load()) throw std::invalid_argument("goicp_estimate_normals: not while a registration runs");
	DeviceGuard guard(dev_);
	const size_t rows = n * (size_t)(k - 1);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_), d_nrm(3 * n), d_var(out_variation ? n : 0);
	Buf<int32_t> d_idx(rows);
	StatReport rep;
	HIPCHK(launch_estimate_normals(d_xyz, (int)n, plan.frames.data(), plan.r2.data(), (int)plan.frames.size(), k, vp, d_nrm,
	                               out_variation ? d_var.get() : nullptr, d_idx, &rep, stream_, ev0_, ev1_));
	HIPCHK(hipMemcpyAsync(out_normals, d_nrm, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, stream_));
	if (out_variation) HIPCHK(hipMemcpyAsync(out_variation, d_var, sizeof(float) * n, hipMemcpyDeviceToHost, stream_));
	if (out_index) HIPCHK(hipMemcpyAsync(out_index, d_idx, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	if (p_.verbose) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		stat_report_line("estimate_normals", n, (int)n, rep);
		std::fprintf(stderr, "[goicp] estimate_normals: k %d, device %.3f ms\n", k, ms);
	}
}

// ---- FPFH descriptors and descriptor matching ----
void Engine::fpfh(const float* xyz, const float* normals, size_t n, int32_t k, float* out_fpfh, uint8_t* out_spfh_counts)
{
	if (!out_fpfh) throw std::invalid_argument("goicp_fpfh: out_fpfh must be non-null");
	knn_self_check_params(n, k);
	const StatPlan plan = StatPlan::of_host_cloud(xyz, n, k);
	fpfh_check_normals(normals, n);
	if (registering_.load()) throw std::invalid_argument("goicp_fpfh: not while a registration runs");
	DeviceGuard guard(dev_);
	const size_t rows = n * (size_t)k, words = n * (size_t)kFpfhDim;
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_), d_nrm = upload_cloud(normals, n, stream_), d_d2(rows), d_out(words);
	Buf<int32_t> d_idx(rows);
	Buf<unsigned char> d_cnt(words);
	StatReport rep;
	HIPCHK(launch_fpfh(d_xyz, d_nrm, (int)n, plan.frames.data(), plan.r2.data(), (int)plan.frames.size(), k, d_idx, d_d2, d_cnt, d_out, &rep, stream_, ev0_, ev1_));
	HIPCHK(hipMemcpyAsync(out_fpfh, d_out, sizeof(float) * words, hipMemcpyDeviceToHost, stream_));
	if (out_spfh_counts) HIPCHK(hipMemcpyAsync(out_spfh_counts, d_cnt, words, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	if (p_.verbose) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		stat_report_line("fpfh", n, (int)n, rep);
		std::fprintf(stderr, "[goicp] fpfh: k %d, device %.3f ms\n", k, ms);
	}
}

void Engine::match_features(const float* q, size_t nq, const float* t, size_t nt, int32_t* out_index, float* out_d2, float* out_d2_second, uint8_t* out_mutual)
{
	if (!out_index || !out_d2 || !out_d2_second) throw std::invalid_argument("goicp_match_features: out_index, out_d2 and out_d2_second must be non-null");
	match_check_descriptors(q, nq, t, nt);
	if (registering_.load()) throw std::invalid_argument("goicp_match_features: not while a registration runs");
	DeviceGuard guard(dev_);
	Buf<float> d_q((size_t)kFpfhDim * nq), d_t((size_t)kFpfhDim * nt), d_d2(nq), d_second(nq);
	Buf<int32_t> d_idx(nq);
	Buf<unsigned char> d_mut(out_mutual ? nq : 0);
	HIPCHK(hipMemcpyAsync(d_q, q, sizeof(float) * kFpfhDim * nq, hipMemcpyHostToDevice, stream_));
	HIPCHK(hipMemcpyAsync(d_t, t, sizeof(float) * kFpfhDim * nt, hipMemcpyHostToDevice, stream_));
	HIPCHK(launch_match_features(d_q, (int)nq, d_t, (int)nt, d_idx, d_d2, d_second, out_mutual ? d_mut.get() : nullptr, stream_, ev0_, ev1_));
	HIPCHK(hipMemcpyAsync(out_index, d_idx, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(out_d2, d_d2, sizeof(float) * nq, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(out_d2_second, d_second, sizeof(float) * nq, hipMemcpyDeviceToHost, stream_));
	if (out_mutual) HIPCHK(hipMemcpyAsync(out_mutual, d_mut, nq, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	if (p_.verbose) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		std::fprintf(stderr, "[goicp] match_features: %zu x %zu, device %.3f ms\n", nq, nt, ms);
	}
}

// ---- symmetric point-to-plane ICP: the source normals ----
void Engine::build_source_normals(const float* h_xyz, const float* d_xyz, const int32_t* d_perm)
{
	const int k = source_normal_k_;
	normals_check_params(N_, k, nullptr);
	const double t0 = now_ms();
	const StatPlan plan = StatPlan::of_host_cloud(h_xyz, N_, k - 1);
	Buf<float> d_up(d_xyz ? 0 : 3 * N_), d_nrm(3 * N_);
	Buf<int32_t> d_idx(N_ * (size_t)(k - 1)), d_pu(d_perm ? 0 : N_);
	StatReport rep;
	if (!d_xyz) {
		HIPCHK(hipMemcpyAsync(d_up, h_xyz, sizeof(float) * 3 * N_, hipMemcpyHostToDevice, stream_));
		d_xyz = d_up.get();
	}
	if (!d_perm) {
		HIPCHK(hipMemcpyAsync(d_pu, src_perm_.data(), sizeof(int32_t) * N_, hipMemcpyHostToDevice, stream_));
		d_perm = d_pu.get();
	}
	HIPCHK(launch_estimate_normals(d_xyz, (int)N_, plan.frames.data(), plan.r2.data(), (int)plan.frames.size(), k, nullptr, d_nrm, nullptr, d_idx, &rep, stream_));
	d_src_normals_.reserve(N_);
	HIPCHK(launch_source_normals_gather(d_nrm, d_perm, (int)N_, d_src_normals_, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	src_normals_k_ = k;
	src_normals_user_ = false;
	source_normal_build_ms_ = now_ms() - t0;
	if (p_.verbose) std::fprintf(stderr, "[goicp] source normals (k = %d, %zu points): %.2f ms\n", k, N_, source_normal_build_ms_);
}

void Engine::ensure_source_normals()
{
	if (src_normals_user_ || (src_normals_k_ == source_normal_k_ && d_src_normals_)) return;
	DeviceGuard guard(dev_);
	// the cloud as the handle holds it, back in the caller's point order
	std::vector<float> xyz(3 * N_);
	for (size_t i = 0; i < N_; i++) std::memcpy(&xyz[3 * (size_t)src_perm_[i]], &h_src_sorted_[4 * i], 3 * sizeof(float));
	build_source_normals(xyz.data(), nullptr, nullptr);
}

void Engine::check_symmetric_query(const char* fn) const
{
	if (registering_.load()) throw std::invalid_argument(std::string(fn) + ": not while a registration runs");
}

void Engine::set_icp_symmetric(int enabled, int source_normal_k)
{
	if (enabled != 0 && enabled != 1) throw std::invalid_argument("goicp_set_icp_symmetric: enabled must be 0 or 1");
	if (enabled && icp_generalized_) throw std::invalid_argument("goicp_set_icp_symmetric: the handle's generalized flag is on (goicp_set_icp_generalized)");
	set_normal_form("goicp_set_icp_symmetric", enabled != 0, enabled != 0, icp_generalized_, gicp_eps_, source_normal_k);
}

void Engine::set_icp_generalized(int enabled, float epsilon, int source_normal_k)
{
	if (enabled != 0 && enabled != 1) throw std::invalid_argument("goicp_set_icp_generalized: enabled must be 0 or 1");
	if (!(epsilon >= kGicpEpsMin && epsilon <= 1.f)) throw std::invalid_argument("goicp_set_icp_generalized: epsilon must be in [1e-4, 1]");
	if (enabled && icp_symmetric_) throw std::invalid_argument("goicp_set_icp_generalized: the handle's symmetric flag is on (goicp_set_icp_symmetric)");
	set_normal_form("goicp_set_icp_generalized", enabled != 0, icp_symmetric_, enabled != 0, epsilon, source_normal_k);
}

// enabled: the value the calling setter gives its own flag; symmetric / generalized: both flags after the call
void Engine::set_normal_form(const char* fn, bool enabled, bool symmetric, bool generalized, float epsilon, int source_normal_k)
{
	const std::string f(fn);
	if (source_normal_k < 3 || source_normal_k > kKnnMax) throw std::invalid_argument(f + ": source_normal_k must be in [3, 32]");
	if ((size_t)source_normal_k > N_) throw std::invalid_argument(f + ": source_normal_k exceeds the number of source points");
	if (enabled && p_.trim_fraction > 0.f) throw std::invalid_argument(f + ": this form of ICP with trim_fraction > 0 is not supported");
	check_symmetric_query(fn);
	if (enabled && icp_gated() && gate_min_inliers_ != 0 && gate_min_inliers_ < 6)
		throw std::invalid_argument(f + ": the handle's gate has min_inliers below point-to-plane's floor of 6");
	const int was = source_normals_active() ? icp_kernel_metric() : 0;
	icp_symmetric_ = symmetric;
	icp_generalized_ = generalized;
	gicp_eps_ = epsilon;
	source_normal_k_ = source_normal_k;
	if (source_normals_active()) {
		DeviceGuard guard(dev_);
		ensure_source_normals();
		if (was != icp_kernel_metric()) {
			// the first launch of the form's kernels (code object load) belongs here, not to the first refinement: one frozen pass
			const float I0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z0[3] = {0, 0, 0};
			icp_state_init(I0, Z0, 0.f, 0, 1);
			icp_launch_one();
			HIPCHK(hipStreamSynchronize(stream_));
		}
	}
}

void Engine::source_normals(float* out)
{
	if (!out) throw std::invalid_argument("goicp_source_normals: out must be non-null");
	check_symmetric_query("goicp_source_normals");
	if (!src_normals_user_ && (size_t)source_normal_k_ > N_)
		throw std::invalid_argument("goicp_source_normals: source_normal_k exceeds the number of source points");
	DeviceGuard guard(dev_);
	ensure_source_normals();
	std::vector<float4> n(N_);
	HIPCHK(hipMemcpy(n.data(), d_src_normals_, sizeof(float4) * N_, hipMemcpyDeviceToHost));
	for (size_t i = 0; i < N_; i++) {
		float* o = out + 3 * (size_t)src_perm_[i];         // back to the caller's point order
		o[0] = n[i].x; o[1] = n[i].y; o[2] = n[i].z;
	}
}

void Engine::set_source_normals(const float* normals, size_t n)
{
	if (!normals) throw std::invalid_argument("goicp_set_source_normals: normals must be non-null");
	if (n != N_) throw std::invalid_argument("goicp_set_source_normals: n must be the handle's source count");
	for (size_t i = 0; i < n; i++) {
		const float* v = normals + 3 * i;
		if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) throw std::invalid_argument("goicp_set_source_normals: non-finite normal");
		if (v[0] == 0.f && v[1] == 0.f && v[2] == 0.f) continue;
		const double len = std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
		if (std::fabs(len - 1.0) > 1e-3) throw std::invalid_argument("goicp_set_source_normals: a normal must be zero or of unit length (within 1e-3)");
	}
	check_symmetric_query("goicp_set_source_normals");
	DeviceGuard guard(dev_);
	Buf<float> d_nrm(3 * N_);
	Buf<int32_t> d_perm(N_);
	HIPCHK(hipMemcpyAsync(d_nrm, normals, sizeof(float) * 3 * N_, hipMemcpyHostToDevice, stream_));
	HIPCHK(hipMemcpyAsync(d_perm, src_perm_.data(), sizeof(int32_t) * N_, hipMemcpyHostToDevice, stream_));
	d_src_normals_.reserve(N_);
	HIPCHK(launch_source_normals_gather(d_nrm, d_perm, (int)N_, d_src_normals_, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	src_normals_user_ = true;
	src_normals_k_ = 0;
}

void Engine::cluster(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t* out_label, int32_t* out_sizes, size_t* n_clusters)
{
	if (!out_label || !n_clusters) throw std::invalid_argument("goicp_cluster: out_label and n_clusters must be non-null");
	VoxelFrame f;
	cluster_frame(xyz, n, radius, min_neighbors, &f);
	if (registering_.load()) throw std::invalid_argument("goicp_cluster: not while a registration runs");
	DeviceGuard guard(dev_);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_);
	Buf<int32_t> d_label(n), d_sizes(n);
	int c = 0;
	HIPCHK(launch_cluster(d_xyz, (int)n, f, radius * radius, min_neighbors, d_label, d_sizes, &c, stream_, ev0_, ev1_));
	HIPCHK(hipMemcpyAsync(out_label, d_label, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream_));
	if (out_sizes && c > 0) HIPCHK(hipMemcpyAsync(out_sizes, d_sizes, sizeof(int32_t) * (size_t)c, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	*n_clusters = (size_t)c;
	if (p_.verbose) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		std::fprintf(stderr, "[goicp] cluster: %zu points, %d clusters, device %.3f ms\n", n, c, ms);
	}
}

namespace {

// the cluster selection of a cloud on the device: launch_cluster, the c sizes to the host, cluster_select there, the c keep flags back and
// the compaction.  d_out: room for 3 n floats; d_index / d_out_label may be null.  ms (may be null): the device time of both launchers
void cluster_filter_device(const float* d_in, int n, const VoxelFrame& f, float radius, int32_t min_neighbors, int32_t min_size, int32_t max_clusters,
                           float* d_out, int32_t* d_index, int32_t* d_out_label, int* m, int* c_out, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                           float* ms)
{
	Buf<int32_t> d_label((size_t)n), d_sizes((size_t)n);
	int c = 0;
	float ms0 = 0.f, ms1 = 0.f;
	HIPCHK(launch_cluster(d_in, n, f, radius * radius, min_neighbors, d_label, d_sizes, &c, stream, ev0, ev1));
	HIPCHK(hipEventElapsedTime(&ms0, ev0, ev1));
	*m = 0;
	if (c_out) *c_out = c;
	if (c > 0) {
		std::vector<int32_t> sizes((size_t)c), keep;
		HIPCHK(hipMemcpyAsync(sizes.data(), d_sizes, sizeof(int32_t) * (size_t)c, hipMemcpyDeviceToHost, stream));
		HIPCHK(hipStreamSynchronize(stream));
		cluster_select(sizes.data(), (size_t)c, min_size, max_clusters, &keep);
		// the keep flags take the sizes' place
		HIPCHK(hipMemcpyAsync(d_sizes, keep.data(), sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, stream));
		HIPCHK(launch_cluster_compact(d_in, n, d_label, d_sizes, d_out, d_index, d_out_label, m, stream, ev0, ev1));
		HIPCHK(hipEventElapsedTime(&ms1, ev0, ev1));
	}
	if (ms) *ms = ms0 + ms1;
}

}  // namespace

void Engine::cluster_filter(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t min_size, int32_t max_clusters, float* out_xyz,
                            int32_t* out_index, int32_t* out_label, size_t* m_out)
{
	if (!out_xyz || !m_out) throw std::invalid_argument("goicp_cluster_filter: out_xyz and m must be non-null");
	cluster_check_select(min_size, max_clusters);
	VoxelFrame f;
	cluster_frame(xyz, n, radius, min_neighbors, &f);
	if (registering_.load()) throw std::invalid_argument("goicp_cluster_filter: not while a registration runs");
	DeviceGuard guard(dev_);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_), d_out(3 * n);
	Buf<int32_t> d_idx(out_index ? n : 0), d_lab(out_label ? n : 0);
	int m = 0, c = 0;
	float ms = 0.f;
	cluster_filter_device(d_xyz, (int)n, f, radius, min_neighbors, min_size, max_clusters, d_out, out_index ? d_idx.get() : nullptr,
	                      out_label ? d_lab.get() : nullptr, &m, &c, stream_, ev0_, ev1_, &ms);
	if (m > 0) HIPCHK(hipMemcpyAsync(out_xyz, d_out, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, stream_));
	if (out_index && m > 0) HIPCHK(hipMemcpyAsync(out_index, d_idx, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream_));
	if (out_label && m > 0) HIPCHK(hipMemcpyAsync(out_label, d_lab, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	*m_out = (size_t)m;
	if (p_.verbose) std::fprintf(stderr, "[goicp] cluster_filter: %zu -> %d points of %d clusters, device %.3f ms\n", n, m, c, ms);
}

void Engine::segment_plane(const float* xyz, size_t n, const PlaneSelect& s, int32_t* out_label, PlaneRecord* out_planes, size_t* n_planes)
{
	if (!out_label || !out_planes || !n_planes) throw std::invalid_argument("goicp_segment_plane: out_label, out_planes and n_planes must be non-null");
	plane_check_cloud(xyz, n);
	if (registering_.load()) throw std::invalid_argument("goicp_segment_plane: not while a registration runs");
	DeviceGuard guard(dev_);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_);
	Buf<int32_t> d_label(n);
	PlaneRecord planes[kPlaneMaxPlanes];
	int c = 0, m = 0;
	HIPCHK(launch_segment_plane(d_xyz, (int)n, s, d_label, nullptr, nullptr, planes, &c, &m, stream_, ev0_, ev1_));
	HIPCHK(hipMemcpyAsync(out_label, d_label, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	for (int p = 0; p < c; p++) out_planes[p] = planes[p];
	*n_planes = (size_t)c;
	if (p_.verbose) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		std::fprintf(stderr, "[goicp] segment_plane: %zu points, %d planes, device %.3f ms\n", n, c, ms);
	}
}

void Engine::plane_filter(const float* xyz, size_t n, const PlaneSelect& s, float* out_xyz, int32_t* out_index, PlaneRecord* out_planes, size_t* n_planes,
                          size_t* m_out)
{
	if (!out_xyz || !m_out) throw std::invalid_argument("goicp_plane_filter: out_xyz and m must be non-null");
	plane_check_cloud(xyz, n);
	if (registering_.load()) throw std::invalid_argument("goicp_plane_filter: not while a registration runs");
	DeviceGuard guard(dev_);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_), d_out(3 * n);
	Buf<int32_t> d_idx(out_index ? n : 0);
	PlaneRecord planes[kPlaneMaxPlanes];
	int c = 0, m = 0;
	HIPCHK(launch_segment_plane(d_xyz, (int)n, s, nullptr, d_out, out_index ? d_idx.get() : nullptr, planes, &c, &m, stream_, ev0_, ev1_));
	if (m > 0) HIPCHK(hipMemcpyAsync(out_xyz, d_out, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, stream_));
	if (out_index && m > 0) HIPCHK(hipMemcpyAsync(out_index, d_idx, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	if (out_planes) for (int p = 0; p < c; p++) out_planes[p] = planes[p];
	if (n_planes) *n_planes = (size_t)c;
	*m_out = (size_t)m;
	if (p_.verbose) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		std::fprintf(stderr, "[goicp] plane_filter: %zu -> %d points behind %d planes, device %.3f ms\n", n, m, c, ms);
	}
}

void Engine::ransac_pose(const float* src, size_t n_s, const float* tgt, size_t n_t, const int32_t* corr, size_t M, const RansacPoseSelect& s,
                         RansacPoseRecord* out_poses, size_t* n_poses, uint8_t* out_inlier)
{
	if (!out_poses || !n_poses) throw std::invalid_argument("goicp_ransac_pose: out_poses and n_poses must be non-null");
	ransac_pose_check_input(src, n_s, tgt, n_t, corr, M);
	if (registering_.load()) throw std::invalid_argument("goicp_ransac_pose: not while a registration runs");
	RansacPoseFrame fs = {}, ft = {};
	if (s.refine) {
		ransac_pose_frame(src, corr, M, 0, &fs);
		ransac_pose_frame(tgt, corr, M, 1, &ft);
	}
	DeviceGuard guard(dev_);
	Buf<float> d_src = upload_cloud(src, n_s, stream_), d_tgt = upload_cloud(tgt, n_t, stream_);
	Buf<int32_t> d_corr(2 * M);
	Buf<unsigned char> d_inlier(out_inlier ? M : 0);
	HIPCHK(hipMemcpyAsync(d_corr, corr, sizeof(int32_t) * 2 * M, hipMemcpyHostToDevice, stream_));
	RansacPoseRecord poses[kRansacPoseMaxPoses];
	int c = 0;
	HIPCHK(launch_ransac_pose(d_src, d_tgt, d_corr, (int)M, s, fs, ft, poses, &c, out_inlier ? d_inlier.get() : nullptr, stream_, ev0_, ev1_));
	if (out_inlier) HIPCHK(hipMemcpyAsync(out_inlier, d_inlier, M, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	for (int p = 0; p < c; p++) out_poses[p] = poses[p];
	*n_poses = (size_t)c;
	if (p_.verbose) {
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		std::fprintf(stderr, "[goicp] ransac_pose: %zu correspondences, %d hypotheses, %d poses, device %.3f ms\n", M, s.iterations, c, ms);
	}
}

void Engine::set_source_staged(const char* fn, const float* xyz, size_t n, const SourceStages& st, size_t* n_kept)
{
	const std::string who(fn);
	if (std::isnan(st.voxel) || st.voxel < 0.f) throw std::invalid_argument(who + ": voxel must be 0 (no stage) or a voxel size > 0");
	if (st.stat_neighbors < 0) throw std::invalid_argument(who + ": stat_neighbors must be 0 (no stage) or in 1..64");
	if (std::isnan(st.radius) || st.radius < 0.f) throw std::invalid_argument(who + ": radius must be 0 (no stage) or a radius > 0");
	if (std::isnan(st.cluster_radius) || st.cluster_radius < 0.f) throw std::invalid_argument(who + ": the cluster radius must be 0 (no stage) or a radius > 0");
	// the counts of the cluster stage are refused with that stage off too; every other parameter of a stage that is off is not looked at
	if (st.cluster_min_neighbors < 0) throw std::invalid_argument("goicp cluster: min_neighbors must not be negative");
	cluster_check_select(st.cluster_min_size, st.cluster_max_clusters);
	if (std::isnan(st.plane_distance) || st.plane_distance < 0.f) throw std::invalid_argument(who + ": the plane distance must be 0 (no stage) or a distance > 0");
	const bool has_voxel = st.voxel > 0.f, has_stat = st.stat_neighbors > 0, has_radius = st.radius > 0.f, has_cluster = st.cluster_radius > 0.f;
	const bool has_plane = st.plane_distance > 0.f;
	PlaneSelect plane_sel;
	if (has_plane) plane_sel = plane_check_select(st.plane_distance, st.plane_iterations, st.plane_refine, st.plane_max, st.plane_min_inliers, st.plane_seed);
	if (!has_voxel && !has_stat && !has_radius && !has_plane && !has_cluster) {
		set_source(xyz, n, fn);
		if (n_kept) *n_kept = n;
		return;
	}
	// everything that can refuse comes first: a refused call leaves the engine as it was.  The stages write no member the ABI shows.  The
	// first stage that runs checks the raw cloud and takes its frame (the statistical stage: its bounds) from the host's walk over it; of
	// the later stages the parameters are checked here, and what only their input can show when that input exists, still before the swap
	VoxelFrame f;
	float mn[3], mx[3];
	if (has_voxel) voxel_frame(xyz, n, st.voxel, &f);
	else if (has_stat) stat_check_cloud(xyz, n, mn, mx);
	else if (has_radius) radius_frame(xyz, n, st.radius, st.min_neighbors, &f);
	else if (has_plane) plane_check_cloud(xyz, n);
	else cluster_frame(xyz, n, st.cluster_radius, st.cluster_min_neighbors, &f);
	if (has_stat) stat_check_params(has_voxel ? 65 : n, st.stat_neighbors, st.stat_std_ratio);   // behind the grid: the range of k and the ratio alone
	if (has_radius) radius_check_params(st.radius, st.min_neighbors);
	if (has_cluster) radius_check_params(st.cluster_radius, std::max(st.cluster_min_neighbors, 1));
	if (registering_.load()) throw std::invalid_argument(who + ": not while a registration runs");
	DeviceGuard guard(dev_);
	const double t0 = now_ms();
	TraceRange tr(fn);
	sync_lane_streams();
	// the raw cloud goes up once; each stage reads the one before it on the device; the final cloud comes back for the host mirror
	const Buf<float> d_raw = upload_cloud(xyz, n, stream_);
	Buf<float> d_voxel, d_stat, d_radius, d_plane, d_cluster;
	const float* d_in = d_raw;
	int n_in = (int)n, m = 0, n_clusters = 0, n_planes = 0;
	bool first = true;                                          // d_in is still the raw cloud, which the host has seen
	float ms = 0.f;
	std::string counts = std::to_string(n), times;              // of the verbose line
	// a stage has run: its output is the input of what follows
	auto ran = [&](const char* stage, const Buf<float>& d_out) {
		if (m < 1) throw std::invalid_argument(who + ": the chain keeps no point");
		d_in = d_out;
		n_in = m;
		first = false;
		if (!p_.verbose) return;
		char t[64];
		std::snprintf(t, sizeof(t), "device %s %.3f ms, ", stage, ms);
		counts += " -> " + std::to_string(m);
		times += t;
	};
	// the bounds of an input the host has not seen, as its walk would find them: 24 bytes come back, not the cloud
	auto bounds = [&] { HIPCHK(launch_cloud_minmax(d_in, n_in, mn, mx, stream_)); };
	if (has_voxel) {
		d_voxel.alloc(3 * n);
		HIPCHK(launch_voxel_downsample(d_in, n_in, f, d_voxel, nullptr, &m, stream_, ev0_, ev1_));
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		ran("voxel", d_voxel);
	}
	if (has_stat) {
		// the sample that steers the first radius: from the host's cloud, or 48 KB of the one on the device
		std::vector<float> sample;
		if (first) {
			sample = stat_sample_host(xyz, n);
		} else {
			stat_check_params((size_t)n_in, st.stat_neighbors, st.stat_std_ratio);
			bounds();
			const size_t ns = stat_sample_size((size_t)n_in), stride = (size_t)n_in / ns;
			sample.resize(3 * ns);
			HIPCHK(hipMemcpy2DAsync(sample.data(), 3 * sizeof(float), d_in, 3 * sizeof(float) * stride, 3 * sizeof(float), ns, hipMemcpyDeviceToHost, stream_));
			HIPCHK(hipStreamSynchronize(stream_));
		}
		const StatPlan plan(mn, mx, (size_t)n_in, st.stat_neighbors, sample);
		StatReport rep;
		d_stat.alloc(3 * (size_t)n_in);
		HIPCHK(launch_stat_outlier_removal(d_in, n_in, plan.frames.data(), plan.r2.data(), (int)plan.frames.size(), st.stat_neighbors, st.stat_std_ratio, d_stat,
		                                   nullptr, nullptr, nullptr, &m, &rep, stream_, ev0_, ev1_));
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		if (p_.verbose) stat_report_line((who.substr(6) + " statistical stage").c_str(), (size_t)n_in, m, rep);
		ran("statistical", d_stat);
	}
	if (has_radius) {
		if (!first) {
			bounds();
			radius_frame_of_box(mn, mx, (size_t)n_in, st.radius, st.min_neighbors, &f);
		}
		d_radius.alloc(3 * (size_t)n_in);
		HIPCHK(launch_radius_outlier_removal(d_in, n_in, f, st.radius * st.radius, st.min_neighbors, d_radius, nullptr, nullptr, &m, stream_, ev0_, ev1_));
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		ran("outlier", d_radius);
	}
	if (has_plane) {
		PlaneRecord planes[kPlaneMaxPlanes];
		d_plane.alloc(3 * (size_t)n_in);
		HIPCHK(launch_segment_plane(d_in, n_in, plane_sel, nullptr, d_plane, nullptr, planes, &n_planes, &m, stream_, ev0_, ev1_));
		HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
		ran("plane", d_plane);
	}
	if (has_cluster) {
		if (!first) {
			bounds();
			cluster_frame_of_box(mn, mx, (size_t)n_in, st.cluster_radius, st.cluster_min_neighbors, &f);
		}
		d_cluster.alloc(3 * (size_t)n_in);
		cluster_filter_device(d_in, n_in, f, st.cluster_radius, st.cluster_min_neighbors, st.cluster_min_size, st.cluster_max_clusters, d_cluster, nullptr, nullptr,
		                      &m, &n_clusters, stream_, ev0_, ev1_, &ms);
		ran("cluster", d_cluster);
	}
	check_swap_size((size_t)n_in, fn);
	std::vector<float> kept(3 * (size_t)n_in);
	HIPCHK(hipMemcpyAsync(kept.data(), d_in, sizeof(float) * 3 * (size_t)n_in, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	load_source(kept.data(), (size_t)n_in, true, d_in);
	finish_source_swap();
	if (n_kept) *n_kept = N_;
	if (p_.verbose) {
		if (has_plane) counts += " (" + std::to_string(n_planes) + " planes removed)";
		if (has_cluster) counts += " points of " + std::to_string(n_clusters) + " clusters";
		else counts += " points";
		std::fprintf(stderr, "[goicp] %s: %s, %.2f ms (%sdevice order %.3f ms)\n", fn + 6, counts.c_str(), now_ms() - t0, times.c_str(),
		             p_.morton_sort >= 1 ? source_order_ms_ : 0.0);
	}
}

void Engine::debug_source_order(const float* xyz, size_t n, int mode, int32_t* perm)
{
	if (!perm) throw std::invalid_argument("goicp_debug_source_order: perm must be non-null");
	if (mode < 0 || mode > 2) throw std::invalid_argument("goicp_debug_source_order: mode must be 0, 1 or 2");
	check_source(xyz, n);
	if (registering_.load()) throw std::invalid_argument("goicp_debug_source_order: not while a registration runs");
	DeviceGuard guard(dev_);
	float mn[3] = {0, 0, 0}, ext = 1.f;
	if (mode == 1) source_morton_frame(xyz, n, mn, &ext);
	Buf<float> d_xyz = upload_cloud(xyz, n, stream_);
	Buf<int32_t> d_perm(n);
	HIPCHK(launch_source_order(d_xyz, (int)n, mode, mn, ext, d_perm, stream_));
	HIPCHK(hipMemcpyAsync(perm, d_perm, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
}

// The members release themselves; what is left here is the order: the engine's device current, nothing in flight on its streams, then the
// members in reverse order of declaration (engine.hpp: buffers and events, the streams, and last restore_device_, which puts the
// caller's device back).  Also the path of an init that threw (see the constructor)
Engine::~Engine()
{
	if (!stream_) return;      // init threw before anything was created
	int prev = -1;
	if (hipGetDevice(&prev) == hipSuccess && prev != dev_) { hipSetDevice(dev_); restore_device_.prev = prev; }
	for (int k = 0; k < kMaxLanes; k++) if (lane_stream_[k]) hipStreamSynchronize(lane_stream_[k]);   // lane 0 is the engine's stream
}
Engine::RestoreDevice::~RestoreDevice() { if (prev >= 0) hipSetDevice(prev); }

void Engine::make_lane_stream(int li)
{
	lane_own_[li].create();
	lane_stream_[li] = lane_own_[li];
}

void Engine::ensure_batch(size_t B, size_t K)
{
	if (B > cap_cubes_) {
		size_t cap = std::max<size_t>(B, cap_cubes_ * 2);
		hipStreamSynchronize(stream_);
		cap_cubes_ = 0;       // stays 0 when one of the six throws: the next call allocates all of them again
		d_cubes_.alloc(cap); d_ub_.alloc(cap); d_lb_.alloc(cap);
		h_cubes_.alloc(cap); h_ub_.alloc(cap); h_lb_.alloc(cap);
		cap_cubes_ = cap;
	}
	if (K > cap_rots_) {
		size_t cap = std::max<size_t>(K, cap_rots_ * 2);
		hipStreamSynchronize(stream_);
		cap_rots_ = 0;
		d_rots_.alloc(cap); h_rots_.alloc(cap);
		cap_rots_ = cap;
	}
	size_t need = bounds_scratch_floats((int)std::max<size_t>(B, 1), (int)N_, nullptr, nullptr);
	// the scratch need is not monotone in B (fewer cubes -> more point chunks): size for the worst case
	size_t worst = (size_t)2 * kGroup * (8 * ((cap_cubes_ + kGroup - 1) / kGroup) + 4096);   // groups x (<= 8 + 2048/groups) chunks
	need = std::max(need, worst);
	if (need > d_scratch_.size()) {
		hipStreamSynchronize(stream_);
		d_scratch_.alloc(need);
	}
}

void Engine::upload_rots(const std::vector<Rot9>& rots)
{
	ensure_batch(1, rots.size());
	std::memcpy(h_rots_, rots.data(), sizeof(Rot9) * rots.size());
	HIPCHK(hipMemcpyAsync(d_rots_, h_rots_, sizeof(Rot9) * rots.size(), hipMemcpyHostToDevice, stream_));
}

// ------------------------------------------------------------------------------------------------
// operators
// ------------------------------------------------------------------------------------------------
void Engine::ensure_bounds_scratch(int B, hipStream_t s)
{
	const size_t need = bounds_scratch_floats(B, (int)N_, nullptr, nullptr);
	if (need <= d_scratch_.size()) return;
	// only the two streams that can still be using the old scratch, not the whole device
	HIPCHK(hipStreamSynchronize(stream_));
	if (s && s != stream_) HIPCHK(hipStreamSynchronize(s));
	d_scratch_.alloc(need);
}

const BoundsOrder* Engine::ensure_bounds_order(int B, hipStream_t s)
{
	const int groups = (B + kGroup - 1) / kGroup;
	if (p_.bounds_order <= 0 || groups < p_.bounds_order_min_groups || !bounds_uses_lean(bounds_dt())) return nullptr;
	if (!h_border_note_) { h_border_note_.alloc(1); *h_border_note_.get() = -1; }
	if (p_.bounds_order_reprobe > 0) {
		// unrelated cubes come in streams of equal size: once a pre-pass has left such a batch alone, the next ones take the plain launch untouched
		const long long note = *static_cast<volatile long long*>(h_border_note_.get());
		if (note == (((long long)groups << 1) | 1) && ++border_skipped_ < p_.bounds_order_reprobe) return nullptr;
		border_skipped_ = 0;
	}
	const int max_runs = std::min(std::max(p_.bounds_order_max_runs, 1), kBoundsOrderMaxRuns);
	// alias, order, pairs, then ctl[] on a 128-B line of its own (the buffer's base is aligned far beyond that)
	const size_t items = bounds_order_items(groups, max_runs), ctl_at = (2 * (size_t)groups + 2 * items + kBoundsCtlInts - 1) / kBoundsCtlInts * kBoundsCtlInts;
	const size_t need = ctl_at + kBoundsCtlInts;
	if (need > d_border_.size()) {
		HIPCHK(hipStreamSynchronize(stream_));
		if (s && s != stream_) HIPCHK(hipStreamSynchronize(s));
		d_border_.alloc(need + need / 2);
	}
	// carved for this launch: a stream runs its launches in order, and the buffer only ever grows after the streams were waited for
	border_.mode = p_.bounds_order >= 2 ? 2 : 1;
	border_.min_groups = p_.bounds_order_min_groups; border_.max_runs = max_runs; border_.cell_vox = p_.bounds_order_cell;
	border_.alias = p_.bounds_dedup != 0 ? reinterpret_cast<int*>(d_border_.get()) : nullptr; border_.order = d_border_.get() + groups;
	border_.pairs = reinterpret_cast<int*>(border_.order + groups); border_.ctl = reinterpret_cast<int*>(d_border_.get() + ctl_at);
	border_.host_note = h_border_note_.get();
	border_.cost = d_bcost_.get(); border_.balance = p_.bounds_balance != 0;
	return &border_;
}

void Engine::eval_bounds_dev(const Rot9* d_rots, const CubeRec* d_cubes, int B, float* d_ub, float* d_lb, hipStream_t s, const ParentRec* d_parents)
{
	DeviceGuard guard(dev_);
	ensure_bounds_scratch(B, s);
	if (inliers_ < (int)N_)
		HIPCHK(launch_bounds_trim(d_src_, (int)N_, dt_, d_rots, d_cubes, d_parents, B, inliers_, d_ub, d_lb, s ? s : stream_));
	else
	{
		const BoundsOrder* bo = d_cubes && !d_parents ? ensure_bounds_order(B, s) : nullptr;     // cube batches only: the search's own rounds come ordered (launch_queue_sort)
		HIPCHK(launch_bounds(d_src_, (int)N_, bounds_dt(), d_rots, d_cubes, d_parents, B, d_scratch_, d_ub, d_lb, s ? s : stream_, bo));
		border_form_ = bo ? bo->mode : 0; border_stream_ = s ? s : stream_;
		int groups = 0;
		bounds_scratch_floats(B, (int)N_, &groups, &border_chunks_);
		border_items_ = (groups + 1) / 2;
	}
	cnt_.bounds_launches++;
}

void Engine::debug_bounds_order(int info[3])
{
	DeviceGuard guard(dev_);
	info[0] = border_form_; info[1] = info[2] = 0;
	if (!border_form_) return;
	int ctl[2] = {0, 0};
	HIPCHK(hipStreamSynchronize(border_stream_));
	HIPCHK(hipMemcpy(ctl, border_.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
	info[1] = ctl[1]; info[2] = ctl[0];
}

void Engine::debug_bounds_twins(int info[2])
{
	DeviceGuard guard(dev_);
	info[0] = info[1] = 0;
	if (border_form_ != 2) return;
	HIPCHK(hipStreamSynchronize(border_stream_));
	HIPCHK(hipMemcpy(info, border_.ctl + 2, 2 * sizeof(int), hipMemcpyDeviceToHost));
}

void Engine::debug_bounds_copies(int info[1])
{
	DeviceGuard guard(dev_);
	info[0] = 0;
	if (border_form_ != 2) return;
	HIPCHK(hipStreamSynchronize(border_stream_));
	HIPCHK(hipMemcpy(info, border_.ctl + kBoundsCopies, sizeof(int), hipMemcpyDeviceToHost));
}

void Engine::debug_bounds_balance(int info[26])
{
	DeviceGuard guard(dev_);
	for (int x = 0; x < 26; x++) info[x] = 0;
	HIPCHK(hipStreamSynchronize(stream_));
	if (d_bcost_) HIPCHK(hipMemcpy(info + 9, d_bcost_, 16 * sizeof(int), hipMemcpyDeviceToHost));
	if (border_form_ == 2 && border_chunks_ == 8) {
		HIPCHK(hipStreamSynchronize(border_stream_));
		HIPCHK(hipMemcpy(info, border_.ctl + kBoundsCut, 9 * sizeof(int), hipMemcpyDeviceToHost));
		info[25] = border_.balance && border_.cost ? 1 : 0;
	} else {
		// no pair launch over eight chunks: its mapping was not in use
		int items = border_items_;
		if (border_form_) {
			int ctl[2] = {0, 0};
			HIPCHK(hipStreamSynchronize(border_stream_));
			HIPCHK(hipMemcpy(ctl, border_.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
			if (ctl[1]) items = ctl[0];
		}
		for (int x = 0; x < 9; x++) info[x] = x * items;
	}
}

bool Engine::debug_bounds_xcd_spans(unsigned long long* out)
{
	DeviceGuard guard(dev_);
	const hipError_t e = bounds_xcd_stamps_take(out, border_stream_ ? border_stream_ : stream_);
	if (e == hipErrorNotSupported) return false;
	HIPCHK(e);
	return true;
}

void Engine::reduce_min_dev(const float* d_v, int n, float* d_min, int* d_idx, hipStream_t s)
{
	DeviceGuard guard(dev_);
	HIPCHK(launch_reduce_min(d_v, n, d_min, d_idx, s ? s : stream_));
}

void Engine::eval_bounds_dev_grouped(const Rot9* d_rots, int nrots, const CubeRec* d_cubes, int B, float* d_ub, float* d_lb, hipStream_t s)
{
	DeviceGuard guard(dev_);
	if (inliers_ < (int)N_) { eval_bounds_dev(d_rots, d_cubes, B, d_ub, d_lb, s); return; }     // the trimmed kernel owns whole cubes: nothing to group
	if (nrots < 1 || nrots > 16) throw std::invalid_argument("goicp: grouped bounds take 1..16 rotations");
	ensure_bounds_scratch(B, s);
	void* gs = scratch_bytes(bounds_grouped_scratch_bytes(B, nrots));
	HIPCHK(launch_bounds_grouped(d_src_, (int)N_, bounds_dt(), d_rots, nrots, d_cubes, B, gs, d_scratch_, d_ub, d_lb, s ? s : stream_));
	cnt_.bounds_launches++;
}

float Engine::time_bounds_dev(const Rot9* d_rots, const CubeRec* d_cubes, int B, float* d_ub, float* d_lb, int iters, int grouped_nrots)
{
	DeviceGuard guard(dev_);
	auto once = [&] { if (grouped_nrots > 0) eval_bounds_dev_grouped(d_rots, grouped_nrots, d_cubes, B, d_ub, d_lb, stream_); else eval_bounds_dev(d_rots, d_cubes, B, d_ub, d_lb, stream_); };
	once();   // sizes the scratch
	HIPCHK(hipStreamSynchronize(stream_));
	HIPCHK(hipEventRecord(ev0_, stream_));
	for (int i = 0; i < iters; i++) once();
	HIPCHK(hipEventRecord(ev1_, stream_));
	HIPCHK(hipEventSynchronize(ev1_));
	float ms = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
	return ms / (float)std::max(iters, 1);
}

void Engine::eval_bounds_batch(const float* rots9, size_t K, const CubeRec* cubes, size_t B, float* ub, float* lb)
{
	if (B == 0) return;
	DeviceGuard guard(dev_);
	for (size_t i = 0; i < B; i++)
		if (cubes[i].rot < 0 || (size_t)cubes[i].rot >= K) throw std::invalid_argument("goicp: cube rotation index out of range");
	ensure_batch(B, K);
	std::memcpy(h_rots_, rots9, sizeof(Rot9) * K);
	if (cubes != h_cubes_) std::memcpy(h_cubes_, cubes, sizeof(CubeRec) * B);
	HIPCHK(hipMemcpyAsync(d_rots_, h_rots_, sizeof(Rot9) * K, hipMemcpyHostToDevice, stream_));
	HIPCHK(hipMemcpyAsync(d_cubes_, h_cubes_, sizeof(CubeRec) * B, hipMemcpyHostToDevice, stream_));
	// an unrelated batch (fewer than half of its groups of eight are the children of one expansion) is grouped on the device
	// first: same bits, ~1.6x faster (eval_bounds_dev_grouped); the search's own batches never take this path
	bool grouped = false;
	if (B >= 256 && K <= 16 && inliers_ >= (int)N_) {
		size_t sib = 0;
		for (size_t g = 0; g + 8 <= B; g += 8) {
			const CubeRec* c = h_cubes_ + g;
			bool s = true;
			for (int j = 1; j < 8 && s; j++)
				s = c[j].rot == c[0].rot && c[j].delta == c[0].delta && c[j].coeff == c[0].coeff && c[j].tx == c[j & 1].tx && c[j].ty == c[j & 2].ty && c[j].tz == c[j & 4].tz;
			sib += s ? 1 : 0;
		}
		grouped = sib * 2 < B / 8;
	}
	if (grouped) eval_bounds_dev_grouped(d_rots_, (int)K, d_cubes_, (int)B, d_ub_, d_lb_, stream_);
	else eval_bounds_dev(d_rots_, d_cubes_, (int)B, d_ub_, d_lb_, stream_);
	HIPCHK(hipMemcpyAsync(h_ub_, d_ub_, sizeof(float) * B, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(h_lb_, d_lb_, sizeof(float) * B, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	if (ub && ub != h_ub_) std::memcpy(ub, h_ub_, sizeof(float) * B);
	if (lb && lb != h_lb_) std::memcpy(lb, h_lb_, sizeof(float) * B);
	cnt_.cubes += (long long)B;
}

void Engine::eval_bounds(const float R[9], const float* cubes4, size_t B, int level, float* ub, float* lb)
{
	if (B == 0) return;
	DeviceGuard guard(dev_);
	ensure_batch(B, 1);
	const float coeff = rot_coeff(level);
	for (size_t i = 0; i < B; i++) {
		CubeRec& c = h_cubes_[i];
		c.tx = cubes4[4 * i]; c.ty = cubes4[4 * i + 1]; c.tz = cubes4[4 * i + 2];
		c.delta = (float)(kSQRT3 / 2.0 * (double)cubes4[4 * i + 3]);   // jly_goicp.cpp:263
		c.coeff = coeff;
		c.rot = 0;
	}
	eval_bounds_batch(R, 1, h_cubes_, B, ub, lb);
}

float Engine::eval_sse(const float R[9], const float t[3])
{
	// sum_i Distance(R p_i + t)^2 (jly_goicp.cpp:100-129): one cube with centre t, no radii
	float cube[4] = {t[0], t[1], t[2], 0.f};
	float ub = 0.f, lb = 0.f;
	struct Exact { bool& f; explicit Exact(bool& x) : f(x) { f = true; } ~Exact() { f = false; } } exact(score_exact_);   // a score, not a bound: fp32 grid
	eval_bounds(R, cube, 1, -1, &ub, &lb);
	cnt_.cubes -= 1;   // a score, not a BnB cube bound
	return ub;
}

void Engine::dt_download(float* out)
{
	DeviceGuard guard(dev_);
	const size_t V = dt_.V;
	if (!dt_.layout) {
		HIPCHK(hipMemcpy(out, d_dt_, sizeof(float) * V * V * V, hipMemcpyDeviceToHost));
		return;
	}
	const size_t VB = dt_.VB, nb = VB * VB * VB * 64;
	std::vector<float> tmp(nb);
	HIPCHK(hipMemcpy(tmp.data(), d_dt_, sizeof(float) * nb, hipMemcpyDeviceToHost));
	for (size_t z = 0; z < V; z++)
		for (size_t y = 0; y < V; y++)
			for (size_t x = 0; x < V; x++) out[(z * V + y) * V + x] = tmp[brick_index(x, y, z, VB)];
}

void Engine::nn_query(const float* q, size_t n, int32_t* idx, float* d2)
{
	if (n == 0) return;
	DeviceGuard guard(dev_);
	// one grow-only scratch block: queries | indices | distances
	char* base = static_cast<char*>(scratch_bytes(sizeof(float) * 5 * n));
	float* dq = reinterpret_cast<float*>(base);
	int32_t* di = reinterpret_cast<int32_t*>(base + sizeof(float) * 3 * n);
	float* dd = reinterpret_cast<float*>(base + sizeof(float) * 4 * n);
	HIPCHK(hipMemcpyAsync(dq, q, sizeof(float) * 3 * n, hipMemcpyHostToDevice, stream_));
	HIPCHK(launch_nn_query(dq, (int)n, kd_, dt_, di, dd, stream_));
	HIPCHK(hipMemcpyAsync(idx, di, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(d2, dd, sizeof(float) * n, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
}

void Engine::knn_query(const float* q, size_t n, int k, int32_t* idx, float* d2)
{
	if (k < 1 || k > kKnnMax || (size_t)k > M_) throw std::invalid_argument("goicp_knn_query: k must be in [1, min(32, M)]");
	if (n == 0) return;
	if (n > (size_t)INT32_MAX / kKnnMax) throw std::invalid_argument("goicp_knn_query: too many queries");
	DeviceGuard guard(dev_);
	// one grow-only scratch block: queries | indices (n x k) | distances (n x k)
	char* base = static_cast<char*>(scratch_bytes(sizeof(float) * 3 * n + (sizeof(int32_t) + sizeof(float)) * n * k));
	float* dq = reinterpret_cast<float*>(base);
	int32_t* di = reinterpret_cast<int32_t*>(base + sizeof(float) * 3 * n);
	float* dd = reinterpret_cast<float*>(base + sizeof(float) * 3 * n + sizeof(int32_t) * n * k);
	HIPCHK(hipMemcpyAsync(dq, q, sizeof(float) * 3 * n, hipMemcpyHostToDevice, stream_));
	HIPCHK(launch_knn_query(dq, (int)n, k, kd_, dt_, di, dd, stream_));
	HIPCHK(hipMemcpyAsync(idx, di, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(d2, dd, sizeof(float) * n * k, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
}

// the accumulator block of the single-pose opt-in iterations (launch_icp_iteration_opt): one for every metric and mode -- each finalize leaves
// it zeroed, and only one of them runs at a time on the engine's stream
void Engine::ensure_icp_acc_opt()
{
	if (d_icp_acc_opt_) return;
	DeviceGuard guard(dev_);
	d_icp_acc_opt_.alloc((size_t)kIcpAccReplicas * kIcpPlaneStride);
	HIPCHK(hipMemsetAsync(d_icp_acc_opt_, 0, sizeof(unsigned long long) * kIcpAccReplicas * kIcpPlaneStride, stream_));
}

void Engine::ensure_normals(int k)
{
	if (normals_k_ == k && d_normals_) return;
	if ((size_t)k > M_) throw std::invalid_argument("goicp_set_icp_options: normal_k exceeds the number of target points");
	DeviceGuard guard(dev_);
	const double t0 = now_ms();
	if (!d_normals_) d_normals_.alloc(M_);
	ensure_icp_acc_opt();
	HIPCHK(hipMemsetAsync(d_normals_, 0, sizeof(float4) * M_, stream_));
	Buf<float> tgt(3 * M_);
	HIPCHK(hipMemcpyAsync(tgt, h_target_.data(), sizeof(float) * 3 * M_, hipMemcpyHostToDevice, stream_));
	HIPCHK(launch_normal_build(tgt, (int)kd_slots_, k, model_centroid_, kd_, dt_, d_normals_, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	normals_k_ = k;
	normal_build_ms_ = now_ms() - t0;
	if (p_.verbose) std::fprintf(stderr, "[goicp] target normals (k = %d): %.2f ms\n", k, normal_build_ms_);
}

void Engine::set_icp_options(int metric, int normal_k)
{
	if (metric != 0 && metric != 1) throw std::invalid_argument("goicp_set_icp_options: metric must be 0 (point-to-point) or 1 (point-to-plane)");
	if (normal_k < 3 || normal_k > kKnnMax) throw std::invalid_argument("goicp_set_icp_options: normal_k must be in [3, 32]");
	if (metric == 1 && p_.trim_fraction > 0.f) throw std::invalid_argument("goicp_set_icp_options: point-to-plane ICP with trim_fraction > 0 is not supported");
	if (registering_.load()) throw std::invalid_argument("goicp_set_icp_options: not while a registration runs");
	if (metric == 1 && icp_gated() && gate_min_inliers_ != 0 && gate_min_inliers_ < 6)
		throw std::invalid_argument("goicp_set_icp_options: the handle's gate has min_inliers below point-to-plane's floor of 6");
	if (metric == 1) {
		ensure_normals(normal_k);
		if (icp_metric_ != 1) {
			// the first launch of the plane kernels (code object load) belongs here, not to the first refinement: one frozen pass
			DeviceGuard guard(dev_);
			const float I0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z0[3] = {0, 0, 0};
			icp_metric_ = 1;
			icp_state_init(I0, Z0, 0.f, 0, 1);
			icp_launch_one();
			HIPCHK(hipStreamSynchronize(stream_));
		}
	}
	icp_metric_ = metric;
	normal_k_ = normal_k;
}

void Engine::set_icp_gate(float max_corr_dist, int min_inliers, int capped_walk)
{
	if (!(max_corr_dist >= 0.f) || !std::isfinite(max_corr_dist)) throw std::invalid_argument("goicp_set_icp_gate: max_corr_dist must be finite and >= 0 (0 = off)");
	if (min_inliers < 0 || (min_inliers != 0 && min_inliers < gate_floor()))
		throw std::invalid_argument("goicp_set_icp_gate: min_inliers must be 0 (the metric's default) or at least 3 (point-to-point) / 6 (point-to-plane)");
	if (capped_walk != 0 && capped_walk != 1) throw std::invalid_argument("goicp_set_icp_gate: capped_walk must be 0 or 1");
	if (registering_.load()) throw std::invalid_argument("goicp_set_icp_gate: not while a registration runs");
	if (max_corr_dist > 0.f) {
		if (icp_robust()) throw std::invalid_argument("goicp_set_icp_gate: a gate together with a robust kernel is not supported (goicp_set_icp_robust kernel 0 first)");
		if (p_.trim_fraction > 0.f || inliers_ < (int)N_) throw std::invalid_argument("goicp_set_icp_gate: a gate together with trim_fraction > 0 is not supported");
		if (dt_.layout == 0 || p_.icp_fused)
			throw std::invalid_argument("goicp_set_icp_gate: the gated pass is fixed-point only (needs dt_layout = 1 and icp_fused = 0)");
		ensure_icp_acc_opt();
	}
	gate_dist_ = max_corr_dist;
	gate_min_inliers_ = min_inliers;
	gate_capped_ = capped_walk;
}

void Engine::set_icp_robust(int kernel, float scale)
{
	if (kernel < 0 || kernel > 4) throw std::invalid_argument("goicp_set_icp_robust: kernel must be 0 (off), 1 Huber, 2 Cauchy, 3 Geman-McClure or 4 Tukey");
	if (kernel != 0 && (!(scale > 0.f) || !std::isfinite(scale))) throw std::invalid_argument("goicp_set_icp_robust: scale must be finite and > 0");
	if (registering_.load()) throw std::invalid_argument("goicp_set_icp_robust: not while a registration runs");
	if (kernel != 0) {
		if (p_.trim_fraction > 0.f || inliers_ < (int)N_) throw std::invalid_argument("goicp_set_icp_robust: a robust kernel together with trim_fraction > 0 is not supported");
		if (icp_gated()) throw std::invalid_argument("goicp_set_icp_robust: a robust kernel together with a gate is not supported (goicp_set_icp_gate max_corr_dist 0 first)");
		if (dt_.layout == 0 || p_.icp_fused)
			throw std::invalid_argument("goicp_set_icp_robust: the robust pass is fixed-point only (needs dt_layout = 1 and icp_fused = 0)");
		ensure_icp_acc_opt();
	}
	robust_kernel_ = kernel;
	robust_scale_ = kernel ? scale : 0.f;
}

void Engine::set_search_truncation(float g)
{
	if (!(g >= 0.f) || !std::isfinite(g)) throw std::invalid_argument("goicp_set_search_truncation: max_dist must be finite and >= 0 (0 = off)");
	if (registering_.load()) throw std::invalid_argument("goicp_set_search_truncation: not while a registration runs");
	if (g > 0.f && (p_.trim_fraction > 0.f || inliers_ < (int)N_))
		throw std::invalid_argument("goicp_set_search_truncation: truncation together with trim_fraction > 0 is not supported");
	dt_.trunc = g;                    // read by the bound launches only (device.hpp DtDesc::trunc)
	if (d_dt16_) dt16_.trunc = g;
}

void Engine::icp_robust_stats(size_t K, float* cost, float* weight_sum) const
{
	if (K == 0 || K != last_robust_cost_.size())
		throw std::invalid_argument("goicp_icp_robust_stats: K must be the pose count of the last goicp_icp_run (1) or goicp_icp_run_batch");
	if (cost) std::memcpy(cost, last_robust_cost_.data(), sizeof(float) * K);
	if (weight_sum) std::memcpy(weight_sum, last_robust_w_.data(), sizeof(float) * K);
}

void Engine::icp_inliers(size_t K, int32_t* out) const
{
	if (!out || K == 0 || K != last_inliers_.size()) throw std::invalid_argument("goicp_icp_inliers: K must be the pose count of the last goicp_icp_run (1) or goicp_icp_run_batch");
	std::memcpy(out, last_inliers_.data(), sizeof(int32_t) * K);
}

void Engine::eval_correspondences(const float R[9], const float t[3], float max_corr_dist, int32_t* index, float* dist_sq, int32_t* inliers, float* sse)
{
	if (!(max_corr_dist >= 0.f) || !std::isfinite(max_corr_dist)) throw std::invalid_argument("goicp_eval_correspondences: max_corr_dist must be finite and >= 0 (0 = no gate)");
	DeviceGuard guard(dev_);
	const float g2 = max_corr_dist > 0.f ? max_corr_dist * max_corr_dist : INFINITY;
	char* base = static_cast<char*>(scratch_bytes((sizeof(int32_t) + sizeof(float)) * N_));
	int32_t* di = reinterpret_cast<int32_t*>(base);
	float* dd = reinterpret_cast<float*>(base + sizeof(int32_t) * N_);
	Pose pose;
	std::memcpy(pose.R, R, sizeof(pose.R));
	std::memcpy(pose.t, t, sizeof(pose.t));
	HIPCHK(launch_eval_correspondences(d_src_, (int)N_, pose, g2, kd_, dt_, di, dd, stream_));
	std::vector<int32_t> hi(N_), oi(N_);
	std::vector<float> hd(N_), od(N_);
	HIPCHK(hipMemcpyAsync(hi.data(), di, sizeof(int32_t) * N_, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(hd.data(), dd, sizeof(float) * N_, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	for (size_t i = 0; i < N_; i++) { oi[(size_t)src_perm_[i]] = hi[i]; od[(size_t)src_perm_[i]] = hd[i]; }   // back to the caller's point order
	int32_t n_in = 0;
	double sum = 0.0;
	for (size_t i = 0; i < N_; i++)
		if (od[i] <= g2) { n_in++; sum += (double)od[i]; }
	if (index) std::memcpy(index, oi.data(), sizeof(int32_t) * N_);
	if (dist_sq) std::memcpy(dist_sq, od.data(), sizeof(float) * N_);
	if (inliers) *inliers = n_in;
	if (sse) *sse = (float)sum;
}

void Engine::target_normals(float* out)
{
	ensure_normals(normal_k_);
	DeviceGuard guard(dev_);
	std::vector<float4> n(M_);
	HIPCHK(hipMemcpy(n.data(), d_normals_, sizeof(float4) * M_, hipMemcpyDeviceToHost));
	for (size_t i = 0; i < M_; i++) { out[3 * i] = n[i].x; out[3 * i + 1] = n[i].y; out[3 * i + 2] = n[i].z; }
}

void Engine::source_transformed(const float R[9], const float t[3], float* out)
{
	// rigid transform apply on the device (kernTransform, src/goicp_kernel.cu:16-22), then back to the
	// caller's point order
	DeviceGuard guard(dev_);
	float4* d_tmp = static_cast<float4*>(scratch_bytes(sizeof(float4) * N_));
	HIPCHK(hipMemcpyAsync(d_tmp, d_src_, sizeof(float4) * N_, hipMemcpyDeviceToDevice, stream_));
	Pose pose;
	std::memcpy(pose.R, R, sizeof(pose.R));
	std::memcpy(pose.t, t, sizeof(pose.t));
	HIPCHK(launch_transform(d_tmp, (int)N_, pose, stream_));
	std::vector<float> h(4 * N_);
	HIPCHK(hipMemcpyAsync(h.data(), d_tmp, sizeof(float4) * N_, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	for (size_t i = 0; i < N_; i++) {
		float* o = out + 3 * (size_t)src_perm_[i];
		o[0] = h[4 * i]; o[1] = h[4 * i + 1]; o[2] = h[4 * i + 2];
	}
}

// ------------------------------------------------------------------------------------------------
// Pose information (goicp_pose_information): one pass of sums on the device, the finishing step in fp64 on the host
// ------------------------------------------------------------------------------------------------
// Eigen-decomposition of a symmetric 6x6 by cyclic Jacobi (fp64), eigenvalues ascending, eigenvectors as rows; rank = the eigenvalues above
// rank_tol * lambda_max (strictly: one exactly at the threshold is dropped); pinv over the retained ones.  A diagonal input is returned as it is.
void information_decompose(const double info[36], double rank_tol, double eig[6], double vec[36], double pinv[36], int32_t* rank)
{
	if (!(rank_tol >= 0.0 && rank_tol < 1.0)) throw std::invalid_argument("goicp_information_decompose: rank_tol must be in [0, 1)");
	double a[6][6], v[6][6];
	for (int i = 0; i < 6; i++)
		for (int j = 0; j < 6; j++) {
			if (!std::isfinite(info[6 * i + j])) throw std::invalid_argument("goicp_information_decompose: the matrix has a non-finite entry");
			a[i][j] = 0.5 * (info[6 * i + j] + info[6 * j + i]);
			v[i][j] = i == j ? 1.0 : 0.0;
		}
	for (int sweep = 0; sweep < 64; sweep++) {
		double off = 0.0;
		for (int i = 0; i < 6; i++)
			for (int j = i + 1; j < 6; j++) off += a[i][j] * a[i][j];
		if (off == 0.0) break;
		for (int p = 0; p < 5; p++)
			for (int q = p + 1; q < 6; q++) {
				if (a[p][q] == 0.0) continue;
				// the rotation that zeroes a[p][q] (Golub & Van Loan, symmetric Schur decomposition)
				const double tau = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
				const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
				const double c = 1.0 / std::sqrt(1.0 + t * t), sn = t * c;
				for (int k = 0; k < 6; k++) {
					const double akp = a[k][p], akq = a[k][q];
					a[k][p] = c * akp - sn * akq;
					a[k][q] = sn * akp + c * akq;
				}
				for (int k = 0; k < 6; k++) {
					const double apk = a[p][k], aqk = a[q][k];
					a[p][k] = c * apk - sn * aqk;
					a[q][k] = sn * apk + c * aqk;
				}
				a[p][q] = a[q][p] = 0.0;
				for (int k = 0; k < 6; k++) {
					const double vkp = v[k][p], vkq = v[k][q];
					v[k][p] = c * vkp - sn * vkq;
					v[k][q] = sn * vkp + c * vkq;
				}
			}
	}
	int order[6] = {0, 1, 2, 3, 4, 5};
	std::stable_sort(order, order + 6, [&](int x, int y) { return a[x][x] < a[y][y]; });
	double lam[6], vr[6][6];
	for (int i = 0; i < 6; i++) {
		lam[i] = a[order[i]][order[i]];
		for (int k = 0; k < 6; k++) vr[i][k] = v[k][order[i]];
	}
	const double thr = rank_tol * lam[5];
	int rk = 0;
	double pi[36] = {0};
	for (int i = 0; i < 6; i++) {
		if (!(lam[i] > thr) || !(lam[i] > 0.0)) continue;
		rk++;
		for (int x = 0; x < 6; x++)
			for (int y = 0; y < 6; y++) pi[6 * x + y] += vr[i][x] * vr[i][y] / lam[i];
	}
	if (eig) std::memcpy(eig, lam, sizeof(lam));
	if (vec) std::memcpy(vec, vr, sizeof(vr));
	if (pinv) std::memcpy(pinv, pi, sizeof(pi));
	if (rank) *rank = rk;
}

void Engine::ensure_pose_info(size_t K)
{
	if (K <= d_info_args_.size()) return;      // the second of the two: it holds K only when both do
	d_info_args_.reset();
	d_info_acc_.alloc((size_t)kIcpBatchAccWords * K);
	d_info_args_.alloc(K);
}

void Engine::pose_information(size_t K, const float* R, const float* t, const goicp_pose_info_options* opt, goicp_pose_info* out, bool batch)
{
	const char* fn = batch ? "goicp_pose_information_batch" : "goicp_pose_information";
	auto refuse = [&](const char* why) { throw std::invalid_argument(std::string(fn) + ": " + why); };
	goicp_pose_info_options o;
	o.metric = -1; o.use_pivot = 0; o.pivot[0] = o.pivot[1] = o.pivot[2] = 0.0; o.rank_tol = kPoseInfoRankTol;
	if (opt) o = *opt;
	if (K == 0 || K > (size_t)kIcpBatchMax) refuse("K must be in [1, 1024]");
	if (!R || !t || !out) refuse("R, t and out must be non-null");
	if (o.metric < -1 || o.metric > 1) refuse("metric must be -1 (the handle's), 0 (point-to-point) or 1 (point-to-plane)");
	if (!(o.rank_tol >= 0.0 && o.rank_tol < 1.0)) refuse("rank_tol must be in [0, 1)");
	for (size_t i = 0; i < 9 * K; i++)
		if (!std::isfinite(R[i])) refuse("R has a non-finite entry");
	for (size_t i = 0; i < 3 * K; i++)
		if (!std::isfinite(t[i])) refuse("t has a non-finite entry");
	if (o.use_pivot)
		for (int i = 0; i < 3; i++)
			if (!std::isfinite(o.pivot[i]) || std::fabs(o.pivot[i]) > 3.0e38) refuse("the pivot has a non-finite entry");
	if (p_.trim_fraction > 0.f || inliers_ < (int)N_) refuse("trim_fraction > 0 is not supported");
	if (dt_.layout == 0 || p_.icp_fused) refuse("the information pass is fixed-point only (needs dt_layout = 1 and icp_fused = 0)");
	if (registering_.load()) refuse("not while a registration runs");
	const int metric = o.metric < 0 ? icp_metric_ : o.metric;
	DeviceGuard guard(dev_);
	if (metric == 1) ensure_normals(normal_k_);
	const int kmetric = kernel_metric(metric);     // the symmetric or generalized form wherever metric 1 is evaluated on a flagged handle
	if (kmetric >= 2) ensure_source_normals();
	if (src_crad_ < 0.0) {
		// largest distance of a source point from the source centroid: with the default pivot |a| <= |R| * this
		double m = 0.0;
		for (size_t i = 0; i < N_; i++) {
			const double dx = (double)h_src_sorted_[4 * i] - src_centroid_[0], dy = (double)h_src_sorted_[4 * i + 1] - src_centroid_[1],
			             dz = (double)h_src_sorted_[4 * i + 2] - src_centroid_[2];
			m = std::max(m, std::sqrt(dx * dx + dy * dy + dz * dz));
		}
		src_crad_ = m;
	}
	std::vector<PoseInfoArgs> args(K);
	for (size_t k = 0; k < K; k++) {
		PoseInfoArgs& a = args[k];
		const float* Rk = R + 9 * k;
		const float* tk = t + 3 * k;
		std::memcpy(a.R, Rk, sizeof(a.R));
		std::memcpy(a.t, tk, sizeof(a.t));
		float c0[3];
		double rho = 0.0, tl = 0.0, off = 0.0;
		for (int i = 0; i < 9; i++) rho += (double)Rk[i] * Rk[i];
		rho = std::sqrt(rho);                          // Frobenius norm: bounds |R x| / |x|
		for (int i = 0; i < 3; i++) {
			c0[i] = Rk[3 * i] * src_centroid_[0] + Rk[3 * i + 1] * src_centroid_[1] + Rk[3 * i + 2] * src_centroid_[2] + tk[i];   // icp_state_fill's cq
			a.c[i] = o.use_pivot ? (float)o.pivot[i] : c0[i];
			tl += (double)tk[i] * tk[i];
			off += ((double)a.c[i] - c0[i]) * ((double)a.c[i] - c0[i]);
		}
		a.g2 = icp_gated() ? gate_dist_ * gate_dist_ : INFINITY;   // icp_state_fill's float product
		a.rk = robust_kernel_;
		a.rc = robust_scale_;
		a.eps = kmetric == 3 ? gicp_eps_ : 0.f;
		// fixed-point scale: |a| <= Ba, |e| <= E, |n| <= 1, so every term is below T^2 with T = 2 (max(Ba, E) + 1), and N of them must fit 2^62
		const double Ba = rho * src_crad_ + std::sqrt(off);
		const double E = rho * (double)src_radius_ + std::sqrt(tl) + std::sqrt(3.0) * (double)target_abs_max_;
		const double T = 2.0 * (std::max(Ba, E) + 1.0);
		const double need = std::log2(4.6e18 / ((double)N_ * T * T));
		if (!std::isfinite(need) || need < -60.0) refuse("the pivot (or the pose) is so far from the clouds that the fixed-point sums would overflow");
		const int e = std::min(60, (int)std::floor(need));
		a.scale = std::ldexp(1.0f, e);
	}
	ensure_pose_info(K);
	const size_t words = (size_t)kIcpBatchAccWords * K;
	HIPCHK(hipMemsetAsync(d_info_acc_, 0, sizeof(unsigned long long) * words, stream_));
	if (batch) {
		HIPCHK(hipMemcpyAsync(d_info_args_, args.data(), sizeof(PoseInfoArgs) * K, hipMemcpyHostToDevice, stream_));
		HIPCHK(launch_pose_info_batch(d_src_, (int)N_, d_info_args_, (int)K, kmetric, kd_, dt_, d_normals_, d_info_acc_, stream_, d_src_normals_));
	} else {
		HIPCHK(launch_pose_info(d_src_, (int)N_, args[0], kmetric, kd_, dt_, d_normals_, d_info_acc_, stream_, d_src_normals_));
	}
	std::vector<long long> acc(words);
	HIPCHK(hipMemcpyAsync(acc.data(), d_info_acc_, sizeof(long long) * words, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	const int nwords = kPoseInfoWords[metric];
	for (size_t k = 0; k < K; k++) {
		long long tot[kIcpPlaneStride] = {0};
		for (int r = 0; r < kIcpAccReplicas; r++)
			for (int w = 0; w < nwords; w++) tot[w] += acc[k * kIcpBatchAccWords + (size_t)r * kIcpPlaneStride + w];   // integers: exact in any order
		const double inv = 1.0 / (double)args[k].scale;      // a power of two
		goicp_pose_info& I = out[k];
		std::memset(&I, 0, sizeof(I));
		double* A = I.information;
		if (metric == 0) {
			const double W = (double)tot[0] / kIcpRobustWScale;
			const double sa[3] = {tot[1] * inv, tot[2] * inv, tot[3] * inv};
			const double xx = tot[4] * inv, xy = tot[5] * inv, xz = tot[6] * inv, yy = tot[7] * inv, yz = tot[8] * inv, zz = tot[9] * inv;
			// A_ww = sum w (|a|^2 I - a a^T), A_wt = sum w [a]x, A_tt = W I
			const double ww[3][3] = {{yy + zz, -xy, -xz}, {-xy, xx + zz, -yz}, {-xz, -yz, xx + yy}};
			const double wt[3][3] = {{0.0, -sa[2], sa[1]}, {sa[2], 0.0, -sa[0]}, {-sa[1], sa[0], 0.0}};
			for (int i = 0; i < 3; i++)
				for (int j = 0; j < 3; j++) {
					A[6 * i + j] = ww[i][j];
					A[6 * i + 3 + j] = wt[i][j];
					A[6 * (3 + j) + i] = wt[i][j];
					A[6 * (3 + i) + 3 + j] = i == j ? W : 0.0;
				}
			for (int i = 0; i < 6; i++) I.gradient[i] = tot[10 + i] * inv;
			I.weight_sum = W; I.cost = tot[16] * inv; I.sse = tot[17] * inv; I.inliers = tot[18];
		} else {
			int w = 0;
			for (int i = 0; i < 6; i++)
				for (int j = i; j < 6; j++) { A[6 * i + j] = A[6 * j + i] = tot[w] * inv; w++; }
			for (int i = 0; i < 6; i++) I.gradient[i] = tot[21 + i] * inv;
			I.cost = tot[27] * inv; I.sse = tot[28] * inv; I.weight_sum = (double)tot[29] / kIcpRobustWScale; I.inliers = tot[30];
		}
		for (int i = 0; i < 3; i++) I.pivot[i] = (double)args[k].c[i];
		I.metric = metric;
		double pinv[36];
		information_decompose(A, o.rank_tol, I.eigenvalues, I.eigenvectors, pinv, &I.rank);
		const double dof = (metric == 0 ? 3.0 : 1.0) * I.weight_sum - 6.0;
		if (dof > 0.0) {
			I.sigma2 = I.cost / dof;
			for (int i = 0; i < 36; i++) I.covariance[i] = I.sigma2 * pinv[i];
		} else {
			I.dof_nonpositive = 1;         // sigma2 and the covariance stay zero
		}
	}
}

void Engine::result_information(const goicp_pose_info_options* opt, goicp_pose_info* out)
{
	if (registering_.load()) throw std::invalid_argument("goicp_result_information: not while a registration runs");
	const Result r = poll();
	if (!r.finished) throw std::invalid_argument("goicp_result_information: the handle has no finished registration");
	pose_information(1, r.optR, r.optT, opt, out, false);
}

// ------------------------------------------------------------------------------------------------
// ICP (ICP3D<float>::Run, jly_icp3d.hpp:181-295; IterativeClosestPoint3D::run, fgoicp/icp3d.cu:83-108)
// The loop state lives on the device (IcpState); iterations are queued in chunks without a host
// round trip, a converged state turns the queued remainder into no-ops.
// ------------------------------------------------------------------------------------------------
void Engine::icp_state_init(const float R[9], const float t[3], float err_diff, int carry_means, int frozen)
{
	icp_cache_active_ = false;          // icp_nn_cache = 2: every run starts with plain walks
	if (source_normals_active()) ensure_source_normals();   // built with the flag, the metric or the swap: a no-op but after set_icp_options(1) on a flagged handle
	icp_state_fill(*h_icp_state_, R, t, err_diff, carry_means, frozen);
	HIPCHK(hipMemcpyAsync(d_icp_state_, h_icp_state_, sizeof(IcpState), hipMemcpyHostToDevice, stream_));
}

void Engine::icp_state_fill(IcpState& st, const float R[9], const float t[3], float err_diff, int carry_means, int frozen) const
{
	std::memset(&st, 0, sizeof(st));
	std::memcpy(st.R, R, sizeof(st.R));
	std::memcpy(st.t, t, sizeof(st.t));
	for (int i = 0; i < 3; i++) {
		st.src_centroid[i] = src_centroid_[i];
		st.cm[i] = model_centroid_[i];
		st.cq[i] = R[3 * i] * src_centroid_[0] + R[3 * i + 1] * src_centroid_[1] + R[3 * i + 2] * src_centroid_[2] + t[i];
	}
	st.err = -1.f;
	st.err_diff_n = err_diff * (float)inliers_;    // jly_icp3d.hpp:255: err_diff * num
	st.n = (float)inliers_;                        // means over the num correspondences used (the reference divides by n, App. B-12)
	st.carry_means = carry_means;
	st.frozen = frozen;
	if (icp_gated()) {
		st.g2 = gate_dist_ * gate_dist_;               // formed once, in float: the pass compares the walk's d^2 with these bits
		st.min_inliers = gate_min_inliers_ ? gate_min_inliers_ : gate_floor();
		st.cost = -1.f;
	}
	if (icp_robust()) {
		st.rk = robust_kernel_;
		st.rc = robust_scale_;
		st.min_inliers = gate_floor();                 // the weight floor: W below it leaves the pose and stops the loop
		st.cost = -1.f;
	}
	{
		// fixed-point scale of the small-cloud pass: every term is a coordinate difference, a product of two, or a squared
		// distance between a moved source point and the target, all below L^2 with L the sum of the extents; N of them must
		// fit 2^62.  ICP moves the cloud towards the target, so the start pose bounds the run.
		const double tl = std::sqrt((double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2]);
		const double L = 2.0 * ((double)src_radius_ + tl + std::sqrt(3.0) * (double)target_abs_max_ + 1.0);
		int e = (int)std::floor(std::log2(4.6e18 / ((double)std::max<size_t>(N_, 1) * L * L)));
		e = std::max(-60, std::min(60, e));
		st.acc_scale = std::ldexp(1.0f, e);
		st.acc_inv = std::ldexp(1.0f, -e);
	}
}

void Engine::icp_launch_one()
{
	// a kernel or a gate, either metric (set_icp_robust / set_icp_gate refuse each other, trimming, the linear DT and the fused iteration), or
	// point-to-plane (set_icp_options refuses it together with trimming)
	if (icp_mode() != kIcpModePlain || icp_metric_ == 1)
		HIPCHK(launch_icp_iteration_opt({d_src_, (int)N_, d_icp_state_, nullptr, 1, icp_kernel_metric(), icp_mode(), d_normals_, d_icp_acc_opt_, gate_capped_, d_src_normals_, gicp_eps_}, kd_, dt_, stream_));
	else if (inliers_ < (int)N_)
		HIPCHK(launch_icp_iteration_trim(d_src_, (int)N_, inliers_, d_icp_state_, kd_, dt_, d_nn_d2_, d_nn_slot_, d_include_, d_icp_partials_, stream_));
	else
		HIPCHK(launch_icp_iteration(d_src_, (int)N_, d_icp_state_, kd_, dt_, d_icp_partials_, p_.icp_fused ? d_icp_ticket_ : nullptr,
		                            (p_.icp_nn_cache == 1 || icp_cache_active_) ? d_nn_cache_ : nullptr, count_hits_ ? d_icp_ticket_ + 8 : nullptr, stream_, d_icp_acc_));
}

// what icp_inliers and icp_robust_stats report, from the final states of a run's K poses
void Engine::icp_last_stats(const IcpState* fin, size_t K)
{
	last_inliers_.resize(K);
	last_robust_cost_.resize(K);
	last_robust_w_.resize(K);
	for (size_t k = 0; k < K; k++) {
		last_inliers_[k] = icp_gated() ? fin[k].n_in : (int32_t)inliers_;
		// without a kernel every weight is 1: C is the pass's err, W is N
		last_robust_cost_[k] = icp_robust() ? fin[k].cost_new : fin[k].err_new;
		last_robust_w_[k] = icp_robust() ? fin[k].w_sum : (float)inliers_;
	}
}

void Engine::icp_state_fetch()
{
	HIPCHK(hipMemcpyAsync(h_icp_state_, d_icp_state_, sizeof(IcpState), hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
}

float Engine::icp_run(float R[9], float t[3], int max_iter, float err_diff, int* iters_out)
{
	DeviceGuard guard(dev_);
	icp_state_init(R, t, err_diff, 1, 0);
	// Chunks of iterations, one chunk ahead: while the host waits for and looks at the state after chunk k, chunk k+1 is
	// already queued, so the GPU never idles between chunks (a blocking fetch per chunk cost ~4 us per iteration on the
	// bunny).  Once the state has converged the queued launches are no-ops (every kernel tests the flag first).
	const int chunk = std::max(1, p_.icp_chunk);
	int queued = 0;
	IcpState* slots = h_icp_state_ + 1;
	hipEvent_t evs[2] = {ev0_, ev1_};
	auto submit = [&](int slot) -> bool {
		if (queued >= max_iter) return false;
		const int k = std::min(chunk, max_iter - queued);
		for (int i = 0; i < k; i++) icp_launch_one();
		queued += k;
		HIPCHK(hipMemcpyAsync(&slots[slot], d_icp_state_, sizeof(IcpState), hipMemcpyDeviceToHost, stream_));
		HIPCHK(hipEventRecord(evs[slot], stream_));
		return true;
	};
	int cur = 0;
	bool have = submit(0);
	const IcpState* fin = nullptr;
	float prev_err = -1.f;
	while (have) {
		const bool next = submit(cur ^ 1);
		HIPCHK(hipEventSynchronize(evs[cur]));
		fin = &slots[cur];
		if (fin->converged || cancel_.load()) break;
		// icp_nn_cache = 2: the exact walk-skipping cache pays once the cloud has nearly stopped moving (the tail of a run: a cached neighbour stays
		// provably nearest for many iterations) and loses while it still moves (every miss is a slower 2-nearest walk) -- so it is switched on, for
		// the chunks queued from here on, when the error fell by less than kIcpCacheRel over the last chunk.  Exact either way: bit-identical states
		if (p_.icp_nn_cache == 2 && d_nn_cache_ && !icp_cache_active_ && prev_err > 0.f && fin->err > 0.f && (prev_err - fin->err) < kIcpCacheRel * fin->err)
			icp_cache_active_ = true;
		prev_err = fin->err;
		have = next;
		cur ^= 1;
	}
	if (fin) *h_icp_state_ = *fin; else icp_state_fetch();      // max_iter <= 0: the state as uploaded
	const IcpState& st = *h_icp_state_;
	std::memcpy(R, st.R, sizeof(st.R));
	std::memcpy(t, st.t, sizeof(st.t));
	if (iters_out) *iters_out = st.iters;
	cnt_.icp_iters += st.passes;
	cnt_.icp_runs++;
	icp_last_stats(&st, 1);
	return st.err_new;
}

void Engine::ensure_icp_batch(size_t K)
{
	if (K <= batch_cap_) return;
	batch_cap_ = 0;
	const size_t cap = std::max<size_t>(K, 16);
	d_batch_states_.alloc(cap);
	h_batch_states_.alloc(3 * cap);
	d_batch_acc_.alloc((size_t)kIcpBatchAccWords * cap);
	HIPCHK(hipMemsetAsync(d_batch_acc_, 0, sizeof(unsigned long long) * kIcpBatchAccWords * cap, stream_));
	d_batch_active_.alloc(2 * cap);
	h_batch_active_.alloc(2 * cap);
	batch_cap_ = cap;
}

// K icp_run loops in one device loop.  Every iteration is one batched pass over the active poses (grid: icp_blocks(N) x active) and one
// finalize wavefront per active pose; pose s has its own IcpState and accumulator block, so its arithmetic is that of icp_run's default
// fixed-point iteration (or of the point-to-plane iteration) bit for bit.  Chunks of icp_chunk iterations are queued one chunk ahead, as in
// icp_run; after each chunk the K states come back, and the next chunk's active list keeps only the poses not yet seen converged (a pose
// that converges inside a chunk already queued turns the rest of it into no-ops, as in icp_run), so the grid shrinks as poses converge.
void Engine::icp_run_batch(size_t K, float* R, float* t, int max_iter, float err_diff, float* err, int32_t* iters)
{
	if (K == 0 || K > (size_t)kIcpBatchMax) throw std::invalid_argument("goicp_icp_run_batch: K must be in [1, 1024]");
	if (!R || !t || max_iter < 0) throw std::invalid_argument("goicp_icp_run_batch: R and t must be non-null and max_iter >= 0");
	if (p_.trim_fraction > 0.f || inliers_ < (int)N_)
		throw std::invalid_argument("goicp_icp_run_batch: trim_fraction > 0 is not supported (a per-pose global selection)");
	if (icp_metric_ == 0 && (dt_.layout == 0 || p_.icp_fused))
		throw std::invalid_argument("goicp_icp_run_batch: point-to-point needs the fixed-point pass of goicp_icp_run (dt_layout = 1, icp_fused = 0)");
	if (registering_.load()) throw std::invalid_argument("goicp_icp_run_batch: not while a registration runs");
	DeviceGuard guard(dev_);
	if (icp_metric_ == 1) ensure_normals(normal_k_);
	if (source_normals_active()) ensure_source_normals();
	ensure_icp_batch(K);
	IcpState* up = h_batch_states_;
	for (size_t k = 0; k < K; k++) icp_state_fill(up[k], R + 9 * k, t + 3 * k, err_diff, 1, 0);
	HIPCHK(hipMemcpyAsync(d_batch_states_, up, sizeof(IcpState) * K, hipMemcpyHostToDevice, stream_));
	const int chunk = std::max(1, p_.icp_chunk);
	int queued = 0, n_active = (int)K;
	std::vector<int> act(K);
	for (size_t k = 0; k < K; k++) act[k] = (int)k;
	IcpState* slots[2] = {h_batch_states_ + batch_cap_, h_batch_states_ + 2 * batch_cap_};
	hipEvent_t evs[2] = {ev0_, ev1_};
	auto submit = [&](int slot) -> bool {
		if (queued >= max_iter || n_active == 0) return false;
		const int k = std::min(chunk, max_iter - queued);
		// this slot's pinned list was last read by the chunk two submissions back, which the host has already waited for
		int* h_act = h_batch_active_ + slot * batch_cap_;
		int* d_act = d_batch_active_ + slot * batch_cap_;
		std::memcpy(h_act, act.data(), sizeof(int) * n_active);
		HIPCHK(hipMemcpyAsync(d_act, h_act, sizeof(int) * n_active, hipMemcpyHostToDevice, stream_));
		for (int i = 0; i < k; i++)
			HIPCHK(launch_icp_iteration_opt({d_src_, (int)N_, d_batch_states_, d_act, n_active, icp_kernel_metric(), icp_mode(), d_normals_, d_batch_acc_, gate_capped_, d_src_normals_, gicp_eps_}, kd_, dt_, stream_));
		queued += k;
		HIPCHK(hipMemcpyAsync(slots[slot], d_batch_states_, sizeof(IcpState) * K, hipMemcpyDeviceToHost, stream_));
		HIPCHK(hipEventRecord(evs[slot], stream_));
		return true;
	};
	int cur = 0;
	bool have = submit(0);
	const IcpState* fin = up;              // max_iter = 0: the states as uploaded
	while (have) {
		const bool next = submit(cur ^ 1);     // one chunk ahead, over the poses not yet seen converged
		HIPCHK(hipEventSynchronize(evs[cur]));
		fin = slots[cur];
		if (cancel_.load()) break;
		n_active = 0;
		for (size_t k = 0; k < K; k++)
			if (!fin[k].converged) act[n_active++] = (int)k;
		if (n_active == 0) break;
		have = next;
		cur ^= 1;
	}
	// a chunk still queued holds only no-ops for the poses seen converged (and, after a cancel, finishes its iterations): the states
	// read back are final once it has drained, and the pinned lists are free again for the next call
	HIPCHK(hipStreamSynchronize(stream_));
	long long passes = 0;
	icp_last_stats(fin, K);
	for (size_t k = 0; k < K; k++) {
		const IcpState& st = fin[k];
		std::memcpy(R + 9 * k, st.R, sizeof(st.R));
		std::memcpy(t + 3 * k, st.t, sizeof(st.t));
		if (err) err[k] = st.err_new;
		if (iters) iters[k] = st.iters;
		passes += st.passes;
	}
	cnt_.icp_iters += passes;
	cnt_.icp_runs += (long long)K;
}

namespace {
uint64_t fnv1a(uint64_t h, const void* p, size_t n)
{
	const unsigned char* b = static_cast<const unsigned char*>(p);
	for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
	return h;
}
// the goicp_status of the exception being handled (the C ABI's mapping, goicp_api.cpp guarded)
int current_status()
{
	try { throw; }
	catch (const StatusError& e) { return e.rc; }
	catch (const std::invalid_argument&) { return GOICP_ERR_INVALID; }
	catch (const std::bad_alloc&) { return GOICP_ERR_INTERNAL; }
	catch (const std::runtime_error&) { return GOICP_ERR_DEVICE; }
	catch (...) { return GOICP_ERR_INTERNAL; }
}
constexpr uint64_t kHealthyWord = ~(uint64_t)0;
}  // namespace

// The sharded ICP loop.  Rank r of G evaluates the workgroups [r B / G, (r+1) B / G) of the world-1 grid of the fixed-point
// pass (B = icp_blocks(N), global N, block offset: every workgroup forms the float row sums of the same 16 queries as at world 1), exports its
// 16 integer totals, and the ranks add them up (mod 2^64: associative, so the world-1 totals bit for bit); every rank then runs the same
// finalize on the same totals and holds the same IcpState -- the same pose, error, iteration count and stop decision, with no collective to
// agree on when to stop.  Per iteration: slice pass -> export -> read back (totals, converged flag, state) -> sum over the ranks -> upload ->
// finalize.  Agreement and failure are collective: one MIN all-reduce of a check word over (R, t, max_iter, err_diff, N, acc_scale, mode)
// first -- as h and ~h, so every rank sees whether all agree -- and a health word in every sum: a rank whose HIP call failed keeps
// exchanging zeros, and all ranks leave in the same iteration.  Trimmed ICP (a global k-selection), the fused iteration and the linear DT
// layout have no fixed-point pass: there every rank runs the full loop replicated (same state everywhere, no sums).
int Engine::icp_run_collective(const goicp_comm_ops* comm, float R[9], float t[3], int max_iter, float err_diff, float* err_out, int* iters_out)
{
	if (!comm || !comm->allreduce_min_u64 || !comm->bcast || comm->world < 1 || comm->rank < 0 || comm->rank >= comm->world || max_iter < 0)
		return GOICP_ERR_INVALID;
	DeviceGuard guard(dev_);
	TraceRange tr("goicp:icp_run_collective");
	const int rank = comm->rank, world = comm->world;
	const bool sliced = inliers_ >= (int)N_ && !p_.icp_fused && dt_.layout != 0 && icp_metric_ == 0 && !icp_gated() && !icp_robust();   // point-to-plane, a gate, a robust kernel: replicated
	IcpShardStats& ss = icp_shard_;
	ss.rank = rank; ss.world = world; ss.sliced = sliced ? 1 : 0;
	ss.blocks = icp_blocks((int)N_);
	ss.block_begin = sliced ? (int)((long long)rank * ss.blocks / world) : 0;
	ss.block_end = sliced ? (int)((long long)(rank + 1) * ss.blocks / world) : ss.blocks;
	ss.runs++;
	int local_rc = GOICP_OK;
	auto local = [&](auto&& f) {
		if (local_rc != GOICP_OK) return;
		try { f(); } catch (...) { local_rc = current_status(); }
	};
	auto health = [&] { return local_rc == GOICP_OK ? kHealthyWord : ((uint64_t)((uint32_t)local_rc + 0x80000000u) << 32) | (uint32_t)rank; };
	auto leave = [&](uint64_t hw) { return local_rc != GOICP_OK ? local_rc : (hw != kHealthyWord ? GOICP_ERR_PEER : GOICP_OK); };

	// agreement: every rank must run the same loop on the same state
	local([&] {
		icp_state_init(R, t, err_diff, 1, 0);
		if (sliced && !h_icp_x_) {
			d_icp_x_.alloc(kIcpExportWords + kIcpAcc);
			h_icp_x_.alloc(kIcpExportWords + kIcpAcc);
		}
	});
	{
		uint64_t h = 0xcbf29ce484222325ull;
		const int32_t ints[5] = {max_iter, (int32_t)N_, sliced ? 1 : 0, world, icp_metric_};
		h = fnv1a(h, R, sizeof(float) * 9);
		h = fnv1a(h, t, sizeof(float) * 3);
		h = fnv1a(h, &err_diff, sizeof(err_diff));
		h = fnv1a(h, ints, sizeof(ints));
		h = fnv1a(h, &h_icp_state_->acc_scale, sizeof(float));
		if (icp_gated()) {                             // the gate joins the check word (an ungated handle hashes what it always did)
			const int32_t gi[2] = {gate_min_inliers_ ? gate_min_inliers_ : gate_floor(), gate_capped_};
			h = fnv1a(h, &gate_dist_, sizeof(float));
			h = fnv1a(h, gi, sizeof(gi));
		}
		if (icp_robust()) {                            // so do the robust kernel and its scale
			h = fnv1a(h, &robust_kernel_, sizeof(robust_kernel_));
			h = fnv1a(h, &robust_scale_, sizeof(float));
		}
		if (icp_symmetric_) {                          // and the symmetric flag with its source_normal_k
			const int32_t si[2] = {1, source_normal_k_};
			h = fnv1a(h, si, sizeof(si));
		}
		if (icp_generalized_) {                        // and the generalized flag with epsilon's bits and its source_normal_k
			int32_t gi[3] = {2, 0, source_normal_k_};
			std::memcpy(&gi[1], &gicp_eps_, sizeof(float));
			h = fnv1a(h, gi, sizeof(gi));
		}
		uint64_t w[3] = {h, ~h, health()};
		const int rc = comm->allreduce_min_u64(comm->ctx, w, 3);
		if (rc != GOICP_OK) return rc;
		ss.collectives++;
		if (w[2] != kHealthyWord) return leave(w[2]);
		if (w[0] != ~w[1]) throw StatusError(GOICP_ERR_INVALID, "goicp_icp_run_collective: the ranks were called with different arguments (pose, max_iter, err_diff, ICP metric, symmetric or generalized flag, gate, robust kernel or scale) or clouds");
	}

	const long long passes0 = cnt_.icp_iters;
	if (!sliced) {
		// fallback: the full loop on every rank, then one exchange of the health words so that every rank returns the same verdict
		int it = 0;
		float e = 0.f;
		local([&] { e = icp_run(R, t, max_iter, err_diff, &it); });
		uint64_t w = health();
		const int rc = comm->allreduce_min_u64(comm->ctx, &w, 1);
		if (rc != GOICP_OK) return rc;
		ss.collectives++;
		if (w != kHealthyWord) return leave(w);
		ss.passes += cnt_.icp_iters - passes0;
		ss.queries += (long long)N_ * (cnt_.icp_iters - passes0);
		if (err_out) *err_out = e;
		if (iters_out) *iters_out = it;
		return GOICP_OK;
	}

	const long long per_pass = icp_slice_queries((int)N_, ss.block_begin, ss.block_end);
	float4* cache = p_.icp_nn_cache == 1 ? d_nn_cache_ : nullptr;
	int* hits = count_hits_ ? d_icp_ticket_ + 8 : nullptr;
	long long* d_up = d_icp_x_ + kIcpExportWords;
	long long* h_up = h_icp_x_ + kIcpExportWords;
	constexpr int kWords = kIcpAcc + 2;          // 16 totals, converged flag, failed-rank count
	for (int k = 0; k <= max_iter; k++) {
		// k == max_iter: no pass, only the read-back of the final state (the totals are zero)
		const double t0 = now_ms();
		local([&] {
			if (k < max_iter)
				HIPCHK(launch_icp_pass_slice(d_src_, (int)N_, ss.block_begin, ss.block_end, d_icp_state_, kd_, dt_, d_icp_acc_, cache, hits, stream_));
			HIPCHK(launch_icp_acc_export(d_icp_acc_, d_icp_state_, d_icp_x_, stream_));
			HIPCHK(hipMemcpyAsync(h_icp_x_, d_icp_x_, sizeof(long long) * kIcpExportWords, hipMemcpyDeviceToHost, stream_));
			HIPCHK(hipStreamSynchronize(stream_));
		});
		int64_t w[kWords] = {};
		if (local_rc == GOICP_OK) {
			std::memcpy(w, h_icp_x_, sizeof(int64_t) * kIcpAcc);
			w[kIcpAcc] = h_icp_x_[kIcpAcc] != 0;
		} else {
			w[kIcpAcc + 1] = 1;
		}
		const double t1 = now_ms();
		ss.round_trip_ms += t1 - t0;
		const int rc = comm_allreduce_sum_i64(comm, w, kWords);
		ss.sum_wait_ms += now_ms() - t1;
		if (rc != GOICP_OK) return rc;
		ss.collectives++;
		if (w[kIcpAcc + 1] != 0) return local_rc != GOICP_OK ? local_rc : GOICP_ERR_PEER;
		if (w[kIcpAcc] != 0 || k == max_iter) break;    // identical states: every rank stops here
		const double t2 = now_ms();
		local([&] {
			std::memcpy(h_up, w, sizeof(int64_t) * kIcpAcc);
			HIPCHK(hipMemcpyAsync(d_up, h_up, sizeof(int64_t) * kIcpAcc, hipMemcpyHostToDevice, stream_));
			HIPCHK(launch_icp_finalize_from_sums(d_up, d_icp_state_, stream_));
		});
		ss.round_trip_ms += now_ms() - t2;
	}
	std::memcpy(h_icp_state_, h_icp_x_ + kIcpAcc + 1, sizeof(IcpState));
	const IcpState& st = *h_icp_state_;
	std::memcpy(R, st.R, sizeof(st.R));
	std::memcpy(t, st.t, sizeof(st.t));
	if (err_out) *err_out = st.err_new;
	if (iters_out) *iters_out = st.iters;
	cnt_.icp_iters += st.passes;
	cnt_.icp_runs++;
	ss.passes += st.passes;
	ss.queries += per_pass * st.passes;
	return GOICP_OK;
}

float Engine::refine_collective(float R[9], float t[3])
{
	ScopedMs acc{icp_ms_};
	int it = 0;
	float e = 0.f;
	const int rc = icp_run_collective(icp_comm_, R, t, p_.icp_max_iter, icp_err_diff_, &e, &it);
	if (rc != GOICP_OK) throw StatusError(rc, "collective ICP refinement failed (status " + std::to_string(rc) + ")");
	unrefined_ = false;
	return eval_sse(R, t);
}

float Engine::time_icp_pass(const float R[9], const float t[3], int iters, bool cached)
{
	DeviceGuard guard(dev_);
	// frozen state: every pass does the same work.  cached = false: the neighbour cache is bypassed, every query walks the
	// tree (the cost of a pass at a new pose); cached = true: the pose repeats, so after the first pass every query hits
	const int keep = p_.icp_nn_cache;
	struct Restore { int& r; int v; ~Restore() { r = v; } } restore{p_.icp_nn_cache, keep};
	if (!cached) p_.icp_nn_cache = 0;
	else if (!d_nn_cache_) throw std::invalid_argument("goicp: the neighbour cache is disabled for this engine");
	else p_.icp_nn_cache = 1;
	icp_state_init(R, t, 0.f, 0, 1);
	icp_launch_one();
	HIPCHK(hipStreamSynchronize(stream_));
	HIPCHK(hipEventRecord(ev0_, stream_));
	for (int i = 0; i < iters; i++) icp_launch_one();
	HIPCHK(hipEventRecord(ev1_, stream_));
	HIPCHK(hipEventSynchronize(ev1_));
	float ms = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
	return ms / (float)std::max(iters, 1);
}

double Engine::probe_gather(int mode, size_t window_bytes)
{
	DeviceGuard guard(dev_);
	unsigned window = 4096;
	while ((size_t)window * 4 < window_bytes && window < (1u << 30)) window <<= 1;
	const size_t nfl = dt_.layout ? (size_t)dt_.VB * dt_.VB * dt_.VB * 64 : (size_t)dt_.V * dt_.V * dt_.V;
	while ((size_t)window > nfl) window >>= 1;
	if (mode >= 2 && window < 16384u) window = 16384u;          // k runs 256 floats apart need 64 KiB
	int cus = 256;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, dev_) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
	const int blocks = mode == 2 ? cus * 2 : cus * 8, iters = 256;        // mode 2: 64 KiB of LDS per workgroup -> two per CU
	float* sink = static_cast<float*>(scratch_bytes(64));
	HIPCHK(launch_probe_gather(dt_, mode, window, blocks, iters, sink, stream_));   // warm-up
	HIPCHK(hipStreamSynchronize(stream_));
	const int reps = 5;
	HIPCHK(hipEventRecord(ev0_, stream_));
	for (int r = 0; r < reps; r++) HIPCHK(launch_probe_gather(dt_, mode, window, blocks, iters, sink, stream_));
	HIPCHK(hipEventRecord(ev1_, stream_));
	HIPCHK(hipEventSynchronize(ev1_));
	float ms = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
	const double lookups = (double)reps * blocks * 256.0 * iters * 8.0;
	return lookups / ((double)ms * 1e-3);
}

void debug_kabsch(const float H[9], float R[9])
{
	Buf<float> buf(18);
	HIPCHK(hipMemcpy(buf.get(), H, sizeof(float) * 9, hipMemcpyHostToDevice));
	HIPCHK(launch_kabsch_debug(buf.get(), buf.get() + 9, nullptr));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(R, buf.get() + 9, sizeof(float) * 9, hipMemcpyDeviceToHost));
}

void Engine::debug_bounds_tile(const float* rots9, const float* parents4, int nseg, int n, int level, int chunks, float* ub_tile, float* lb_tile,
                               float* ub_direct, float* lb_direct, float ms[2], unsigned stats[2])
{
	DeviceGuard guard(dev_);
	if (nseg < 1 || n < 1 || n > 64 || chunks < 1) throw std::invalid_argument("goicp: debug_bounds_tile: bad shape");
	const size_t G = (size_t)nseg * n, B = G * kGroup;
	struct Seg { int off, n, rot; };
	std::vector<ParentRec> par(G);
	std::vector<Seg> segs((size_t)nseg);
	const float coeff = rot_coeff(level);
	for (int i = 0; i < nseg; i++) {
		segs[(size_t)i] = Seg{i * n, n, i};
		for (int e = 0; e < n; e++) {
			const float* q = parents4 + ((size_t)i * n + e) * 4;
			par[(size_t)i * n + e] = ParentRec{q[0], q[1], q[2], q[3], coeff, i};
		}
	}
	int g2 = 0, c2 = 0;
	const size_t sc_direct = bounds_scratch_floats((int)B, (int)N_, &g2, &c2), sc_tile = G * (size_t)chunks * 2 * kGroup;
	Buf<ParentRec> d_par(G);
	Buf<Seg> d_seg((size_t)nseg);
	Buf<Rot9> d_rot((size_t)nseg);
	Buf<float> d_out(4 * B), d_sc(std::max(sc_direct, sc_tile) + 64);
	Buf<unsigned> d_stats(2);
	HIPCHK(hipMemcpyAsync(d_par.get(), par.data(), sizeof(ParentRec) * G, hipMemcpyHostToDevice, stream_));
	HIPCHK(hipMemcpyAsync(d_seg.get(), segs.data(), sizeof(Seg) * (size_t)nseg, hipMemcpyHostToDevice, stream_));
	HIPCHK(hipMemcpyAsync(d_rot.get(), rots9, sizeof(Rot9) * (size_t)nseg, hipMemcpyHostToDevice, stream_));
	HIPCHK(hipMemsetAsync(d_stats.get(), 0, sizeof(unsigned) * 2, stream_));
	float* t_ub = d_out.get(); float* t_lb = d_out.get() + B; float* r_ub = d_out.get() + 2 * B; float* r_lb = d_out.get() + 3 * B;
	const int reps = 5;
	for (int pass = 0; pass < 2; pass++) {              // pass 0 warms up (and counts the sub-patches), pass 1 is timed
		HIPCHK(hipEventRecord(ev0_, stream_));
		for (int r = 0; r < (pass ? reps : 1); r++)
			HIPCHK(launch_bounds_tile(d_src_, (int)N_, dt_, d_rot.get(), d_par.get(), d_seg.get(), nseg, n, chunks, d_sc.get(), t_ub, t_lb, pass ? nullptr : d_stats.get(), stream_));
		HIPCHK(hipEventRecord(ev1_, stream_));
		HIPCHK(hipEventSynchronize(ev1_));
		if (pass) { HIPCHK(hipEventElapsedTime(&ms[0], ev0_, ev1_)); ms[0] /= reps; }
	}
	for (int pass = 0; pass < 2; pass++) {
		HIPCHK(hipEventRecord(ev0_, stream_));
		for (int r = 0; r < (pass ? reps : 1); r++)
			HIPCHK(launch_bounds(d_src_, (int)N_, dt_, d_rot.get(), nullptr, d_par.get(), (int)B, d_sc.get(), r_ub, r_lb, stream_));
		HIPCHK(hipEventRecord(ev1_, stream_));
		HIPCHK(hipEventSynchronize(ev1_));
		if (pass) { HIPCHK(hipEventElapsedTime(&ms[1], ev0_, ev1_)); ms[1] /= reps; }
	}
	HIPCHK(hipMemcpy(ub_tile, t_ub, sizeof(float) * B, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(lb_tile, t_lb, sizeof(float) * B, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(ub_direct, r_ub, sizeof(float) * B, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(lb_direct, r_lb, sizeof(float) * B, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(stats, d_stats.get(), sizeof(unsigned) * 2, hipMemcpyDeviceToHost));
}

// What the two queue-round test entries share.  Set-up: the rotation, two searches (0: the upper-bound pass, coeff 0; 1: the lower-bound pass of
// rotation level `level`) whose queues hold exactly the first cnt[s] of the given nodes (lower bound 0: all of them pass the stop rule against a
// huge incumbent and, cnt <= K, all are selected; the list keeps the queue order), and a zeroed control block.  -> the twin lists are in use
bool Engine::debug_queue_setup(QLane& L, const float R[9], int level, const float* parents4, const int cnt[2])
{
	std::vector<Rot9> rot(1);
	std::memcpy(rot[0].r, R, sizeof(float) * 9);
	upload_rots(rot);
	const bool twins = p_.twin_fusion && L.d_psearch[0] != nullptr;
	const int n = std::max(cnt[0], cnt[1]);
	std::vector<QNode> nodes((size_t)n);
	for (int i = 0; i < n; i++) nodes[(size_t)i] = QNode{parents4[4 * i], parents4[4 * i + 1], parents4[4 * i + 2], parents4[4 * i + 3], 0.f, 0.f};
	for (int s = 0; s < 2; s++) {
		QSearch& q = L.h_search[s];
		std::memset(&q, 0, sizeof(q));
		q.best = 1e30f; q.coeff = s ? rot_coeff(level) : 0.f; q.rot = 0; q.count = cnt[s]; q.min_ub = INFINITY; q.twin = twins ? (s ^ 1) : -1;
		HIPCHK(hipMemcpyAsync(L.d_nodes + (size_t)s * kQueueCap, nodes.data(), sizeof(QNode) * (size_t)cnt[s], hipMemcpyHostToDevice, stream_));
	}
	HIPCHK(hipMemcpyAsync(L.d_search, L.h_search, sizeof(QSearch) * 2, hipMemcpyHostToDevice, stream_));
	std::memset(L.h_ctl, 0, sizeof(QCtl));
	L.h_ctl->tile_chunks = 1;
	HIPCHK(hipMemcpyAsync(L.d_ctl, L.h_ctl, sizeof(QCtl), hipMemcpyHostToDevice, stream_));
	return twins;
}

// the control block and the searches after the round
void Engine::debug_queue_fetch(QLane& L)
{
	HIPCHK(hipMemcpyAsync(L.h_ctl, L.d_ctl, sizeof(QCtl), hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(L.h_search, L.d_search, sizeof(QSearch) * 2, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
}

// Read-back: the children's bounds of both searches from the list they were evaluated in (`total` expansions; L.h_search[s].parent_off places
// search s), in the order of parents4.  chunks > 1: the chunk partials of d_scratch are added here in chunk order -- in float, as the next
// round's digest does (exact_sum false), or in double and rounded once, so that what comes back is the evaluation's error and not this sum's
void Engine::debug_queue_gather(QLane& L, const ParentRec* d_list, int total, int chunks, const float* d_scratch, const float* d_ub, const float* d_lb, bool exact_sum,
                                const float* parents4, const int cnt[2], float* const out[4])
{
	std::vector<ParentRec> listed((size_t)total);
	HIPCHK(hipMemcpy(listed.data(), d_list, sizeof(ParentRec) * (size_t)total, hipMemcpyDeviceToHost));
	std::vector<float> ub((size_t)kGroup * total), lb((size_t)kGroup * total), part;
	if (chunks > 1) {
		part.resize((size_t)total * chunks * 2 * kGroup);
		HIPCHK(hipMemcpy(part.data(), d_scratch, sizeof(float) * part.size(), hipMemcpyDeviceToHost));
	} else {
		HIPCHK(hipMemcpy(ub.data(), d_ub, sizeof(float) * ub.size(), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(lb.data(), d_lb, sizeof(float) * lb.size(), hipMemcpyDeviceToHost));
	}
	for (int s = 0; s < 2; s++) {
		const int off = L.h_search[s].parent_off;
		if (off < 0 || off + cnt[s] > total) throw std::logic_error("goicp: debug queue round: a search's expansions lie outside the list");
		float* ou = out[2 * s]; float* ol = out[2 * s + 1];
		for (int e = 0; e < cnt[s]; e++) {
			const ParentRec& pr = listed[(size_t)off + e];
			if (pr.x != parents4[4 * e] || pr.y != parents4[4 * e + 1] || pr.z != parents4[4 * e + 2] || pr.w != parents4[4 * e + 3])
				throw std::logic_error("goicp: debug queue round: the list is not in queue order");
			for (int c = 0; c < kGroup; c++) {
				if (chunks > 1) {
					const float* sp = part.data() + (size_t)(off + e) * chunks * (2 * kGroup);
					if (exact_sum) {
						double a = 0.0, b = 0.0;
						for (int j = 0; j < chunks; j++) { a += (double)sp[(size_t)j * 2 * kGroup + c]; b += (double)sp[(size_t)j * 2 * kGroup + kGroup + c]; }
						ou[8 * e + c] = (float)a; ol[8 * e + c] = (float)b;
					} else {
						float a = 0.f, b = 0.f;
						for (int j = 0; j < chunks; j++) { a += sp[(size_t)j * 2 * kGroup + c]; b += sp[(size_t)j * 2 * kGroup + kGroup + c]; }
						ou[8 * e + c] = a; ol[8 * e + c] = b;
					}
				} else { ou[8 * e + c] = ub[(size_t)8 * (off + e) + c]; ol[8 * e + c] = lb[(size_t)8 * (off + e) + c]; }
			}
		}
	}
}

void Engine::debug_queue_expand(const float R[9], int level, const float* parents4, int n, float* ub0, float* lb0, float* ub1, float* lb1, int info[2])
{
	DeviceGuard guard(dev_);
	if (n < 1 || n > kQueueRoundPop) throw std::invalid_argument("goicp: debug_queue_expand takes 1..128 nodes");
	if (!(p_.device_queues && p_.trans_batch > 1 && p_.wide_children)) throw std::invalid_argument("goicp: debug_queue_expand needs the device-queue configuration");
	if (inliers_ < (int)N_) throw std::invalid_argument("goicp: debug_queue_expand: untrimmed engines only");
	ensure_lane(0, 2);
	QLane& L = ql_[0];
	const int cnt[2] = {n, n};
	const bool twins = debug_queue_setup(L, R, level, parents4, cnt);
	QParams qp = queue_params();
	qp.K = std::max(n, 1); qp.kmax = kQueueRoundPop; qp.tile_on = 0; qp.stale_widen = 0; qp.stale_compact = 0;
	const int parity = 0, max_groups = 2 * n;
	RoundOpts round;
	round.twins = twins; round.count = false;
	queue_round(L, 2, qp, parity, max_groups, round);
	debug_queue_fetch(L);
	if (L.h_ctl->overflow || L.h_ctl->n_groups[parity] != 2 * n || L.h_search[0].n_parents != n || L.h_search[1].n_parents != n)
		throw std::logic_error("goicp: debug_queue_expand: the round did not list every node");
	const int chunks = L.h_ctl->chunks;
	info[0] = chunks; info[1] = twins ? 1 : 0;
	float* const out[4] = {ub0, lb0, ub1, lb1};
	debug_queue_gather(L, L.d_parents[parity], 2 * n, chunks, L.d_scratch, L.d_ub, L.d_lb, false, parents4, cnt, out);
}

void Engine::debug_queue_expand_tiles(const float R[9], int level, const float* parents4, int n, int n_ub, float* ub0, float* lb0, float* ub1, float* lb1, int info[4],
                                      const QueueDigest* dg)
{
	DeviceGuard guard(dev_);
	if (n < 1 || n > kQueueRoundPop || n_ub < 1 || n_ub > n) throw std::invalid_argument("goicp: debug_queue_expand_tiles takes 1..128 nodes, 1..n of them in the upper-bound search");
	if (!(p_.device_queues && p_.trans_batch > 1 && p_.wide_children)) throw std::invalid_argument("goicp: debug_queue_expand_tiles needs the device-queue configuration");
	if (!tiles_usable()) throw std::invalid_argument("goicp: debug_queue_expand_tiles needs the tile list (lds_tiles, the bricked fp32 grid, no trimming)");
	ensure_lane(0, 2);
	QLane& L = ql_[0];
	if (!L.tile.ub) throw std::logic_error("goicp: debug_queue_expand_tiles: the lane has no tile list");
	const int cnt[2] = {n_ub, n};
	const bool twins = debug_queue_setup(L, R, level, parents4, cnt);
	QParams qp = queue_params();
	qp.K = n; qp.kmax = kQueueRoundPop; qp.stale_widen = 0; qp.stale_compact = 0;
	qp.tile_on = 1; qp.tile_min = 1; qp.tile_spread = 1e30f;              // any selection qualifies, however far apart its nodes lie
	const int parity = 0, total = n_ub + n;
	// every row the evaluation does not write reads back as NaN: an item that never stored its sums cannot pass for one that did
	HIPCHK(hipMemsetAsync(L.tile.scratch, 0xff, sizeof(float) * bounds_tile_queue_scratch_floats(L.seg_cap), stream_));
	HIPCHK(hipMemsetAsync(L.tile.ub, 0xff, sizeof(float) * (size_t)L.list_cap * kGroup, stream_));
	HIPCHK(hipMemsetAsync(L.tile.lb, 0xff, sizeof(float) * (size_t)L.list_cap * kGroup, stream_));
	RoundOpts round;
	round.tiles = true; round.twins = twins; round.count = false;
	queue_round(L, 2, qp, parity, 2 * n, round);
	debug_queue_fetch(L);
	const QCtl& c = *L.h_ctl;
	if (c.overflow || c.n_groups[parity] != 0 || c.n_tile_groups[parity] != total || L.h_search[0].n_parents != n_ub || L.h_search[1].n_parents != n ||
	    L.h_search[0].tile != 1 || L.h_search[1].tile != 1)
		throw std::logic_error("goicp: debug_queue_expand_tiles: the round did not list every node in the tile list");
	const int chunks = c.tile_chunks, nsegs = c.n_tile_segs[parity];
	if (chunks < 1 || nsegs != (n_ub + 63) / 64 + (n + 63) / 64) throw std::logic_error("goicp: debug_queue_expand_tiles: unexpected tile shape");
	info[0] = chunks; info[1] = nsegs; info[2] = bounds_tile_queue_grid(); info[3] = twins ? 1 : 0;
	float* const out[4] = {ub0, lb0, ub1, lb1};
	// (the chunk partials are added in double: up to 342 of them in a test, which a float sum's own rounding would blur)
	debug_queue_gather(L, L.tile.parents[parity], total, chunks, L.tile.scratch, L.tile.ub, L.tile.lb, true, parents4, cnt, out);
	if (!dg) return;
	// the next round's queue kernel alone: it digests the tile list's bounds (S->tile: tile.parents[0], tile.ub / lb or tile.scratch with
	// ctl->tile_chunks) and selects one node per search
	QParams q2 = qp;
	q2.K = 1; q2.tile_on = 0;
	HIPCHK(launch_bnb_queue(L.d_search, L.d_nodes, 2, q2, L.d_parents[0], L.d_parents[1], L.d_ub, L.d_lb, L.d_scratch, L.d_ctl, 1, stream_, &L.tile,
	                        twins ? L.d_psearch[1].get() : nullptr, true));
	HIPCHK(hipMemcpyAsync(L.h_ctl, L.d_ctl, sizeof(QCtl), hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(L.h_search, L.d_search, sizeof(QSearch) * 2, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	if (L.h_ctl->overflow) throw std::logic_error("goicp: debug_queue_expand_tiles: the digest overflowed");
	for (int s = 0; s < 2; s++) {
		const QSearch& S = L.h_search[s];
		// (a search that stopped on the stop rule lists nothing and keeps the flags of its last selection)
		if (S.count < 0 || S.count > 8 * cnt[s] || S.n_parents < 0 || S.n_parents > 1 || (S.n_parents == 1 && S.tile != 0) || (S.n_parents == 0 && S.done != 1))
			throw std::logic_error("goicp: debug_queue_expand_tiles: unexpected queue after the digest");
		dg->counts[2 * s] = S.count; dg->counts[2 * s + 1] = S.n_parents;
		if (S.count > 0) {
			static_assert(sizeof(QNode) == 6 * sizeof(float), "a queue node is six floats");
			HIPCHK(hipMemcpy(dg->nodes + (size_t)s * 8 * n * 6, L.d_nodes + (size_t)s * kQueueCap, sizeof(QNode) * (size_t)S.count, hipMemcpyDeviceToHost));
		}
		float* li = dg->listed + 4 * s;
		li[0] = li[1] = li[2] = li[3] = 0.f;
		if (S.n_parents == 1) {
			ParentRec pr;
			HIPCHK(hipMemcpy(&pr, L.d_parents[1].get() + S.parent_off, sizeof(ParentRec), hipMemcpyDeviceToHost));
			li[0] = pr.x; li[1] = pr.y; li[2] = pr.z; li[3] = pr.w;
		}
		float* so = dg->search + 8 * s;
		so[0] = S.best; so[1] = S.min_ub; so[2] = (float)S.improved; so[3] = S.bx; so[4] = S.by; so[5] = S.bz; so[6] = S.bw; so[7] = (float)S.done;
	}
}

void Engine::debug_queue_round(const goicp_queue_round& rp, goicp_queue_search* searches, float* nodes, const void* prev_parents, const float* prev_ub,
                               const float* prev_lb, const float* prev_scratch, int32_t ctl[6], void* listed, int32_t* parent_search)
{
	static_assert(sizeof(goicp_queue_search) == sizeof(QSearch) && offsetof(goicp_queue_search, twin) == offsetof(QSearch, twin) &&
	              offsetof(goicp_queue_search, min_ub) == offsetof(QSearch, min_ub), "goicp_queue_search is QSearch");
	static_assert(GOICP_QUEUE_SLAB == kQueueCap && sizeof(QNode) == 6 * sizeof(float), "a slab of six-float nodes");
	// everything the kernel turns into an address is checked here: it trusts its host
	const auto bad = [](const char* what) { throw std::invalid_argument(std::string("goicp: debug_queue_round: ") + what); };
	const int ns = rp.nsearch, npl = rp.n_prev_list;
	if (ns < 1 || ns > 8 || (rp.parity != 0 && rp.parity != 1) || (rp.deep != 0 && rp.deep != 1)) bad("nsearch 1..8, parity and deep 0 / 1");
	if (rp.K < 1 || rp.K > kQueueMaxPop || rp.kmax < 1) bad("K 1..512, kmax >= 1");
	if (rp.cap < 1 || rp.cap > kQueueCap) bad("cap 1..8192");
	if (rp.list_cap < 1 || rp.list_cap > 65536 || npl < 0 || npl > rp.list_cap) bad("list_cap 1..65536, n_prev_list 0..list_cap");
	if (rp.chunks < 1 || rp.chunks > 1024) bad("chunks 1..1024");
	if (rp.stale_widen < 0 || rp.stale_widen > 3 || rp.stale_compact < 0 || rp.depth < 0 || rp.tile_min < 0) bad("stale_widen 0..3; stale_compact, depth, tile_min >= 0");
	if (!(rp.root[3] > 0.f) || !std::isfinite(rp.root[3]) || !std::isfinite(rp.thr)) bad("a finite threshold and a positive finite root width");
	if (npl > 0 && (!prev_parents || (rp.chunks == 1 ? !(prev_ub && prev_lb) : !prev_scratch))) bad("the previous list or its bounds are missing");
	if (ctl[rp.parity] < 0 || ctl[rp.parity] > rp.list_cap) bad("n_groups of this parity outside the list");
	for (int s = 0; s < ns; s++) {
		const goicp_queue_search& q = searches[s];
		if (q.count < 0 || q.count > rp.cap) bad("a queue longer than cap");
		if (q.done < 0 || q.done > 2 || q.tile != 0 || q.stale < 0 || q.stale > (1 << 20)) bad("done 0..2, tile 0, stale 0..2^20");
		if (q.n_parents < 0 || q.n_parents > kQueueMaxPop || (q.n_parents > 0 && (q.parent_off < 0 || q.parent_off > npl - q.n_parents)))
			bad("previous expansions outside the previous list");
	}
	DeviceGuard guard(dev_);
	const size_t nprev = (size_t)std::max(npl, 1), ncap = (size_t)rp.list_cap;
	Buf<QSearch> d_search((size_t)ns);
	Buf<QNode> d_nodes((size_t)ns * kQueueCap);
	Buf<ParentRec> d_prev(nprev), d_list(ncap);
	Buf<float> d_ub(nprev * kGroup), d_lb(nprev * kGroup), d_scratch(nprev * (size_t)rp.chunks * 2 * kGroup);
	Buf<int> d_psearch(ncap);
	Buf<QCtl> d_ctl(1);
	QParams qp{};
	qp.thr = rp.thr; qp.K = rp.K; qp.kmax = rp.kmax; qp.list_cap = rp.list_cap; qp.seg_cap = 0;
	qp.root_x = rp.root[0]; qp.root_y = rp.root[1]; qp.root_z = rp.root[2]; qp.root_w = rp.root[3];
	qp.boxed = rp.boxed; qp.depth = rp.depth; qp.cap = rp.cap; qp.soft_overflow = rp.soft_overflow;
	for (int k = 0; k < 3; k++) { qp.lo[k] = rp.lo[k]; qp.hi[k] = rp.hi[k]; }
	qp.tile_on = 0; qp.tile_min = rp.tile_min; qp.tile_spread = rp.tile_spread;
	qp.stale_widen = rp.stale_widen; qp.stale_compact = rp.stale_compact;
	QCtl c{};
	c.n_groups[0] = ctl[0]; c.n_groups[1] = ctl[1]; c.n_active[0] = ctl[2]; c.n_active[1] = ctl[3]; c.overflow = ctl[4]; c.tile_hint = ctl[5];
	c.chunks = rp.chunks; c.tile_chunks = 1;
	// what the kernel does not write reads back as all-ones bits (NaN, -1); so do the bounds the caller did not give
	HIPCHK(hipMemsetAsync(d_list.get(), 0xff, sizeof(ParentRec) * ncap, stream_));
	HIPCHK(hipMemsetAsync(d_psearch.get(), 0xff, sizeof(int) * ncap, stream_));
	HIPCHK(hipMemsetAsync(d_ub.get(), 0xff, sizeof(float) * nprev * kGroup, stream_));
	HIPCHK(hipMemsetAsync(d_lb.get(), 0xff, sizeof(float) * nprev * kGroup, stream_));
	HIPCHK(hipMemsetAsync(d_scratch.get(), 0xff, sizeof(float) * nprev * (size_t)rp.chunks * 2 * kGroup, stream_));
	HIPCHK(hipMemsetAsync(d_prev.get(), 0xff, sizeof(ParentRec) * nprev, stream_));
	if (npl > 0) {
		HIPCHK(hipMemcpyAsync(d_prev.get(), prev_parents, sizeof(ParentRec) * (size_t)npl, hipMemcpyHostToDevice, stream_));
		if (rp.chunks == 1) {
			HIPCHK(hipMemcpyAsync(d_ub.get(), prev_ub, sizeof(float) * (size_t)npl * kGroup, hipMemcpyHostToDevice, stream_));
			HIPCHK(hipMemcpyAsync(d_lb.get(), prev_lb, sizeof(float) * (size_t)npl * kGroup, hipMemcpyHostToDevice, stream_));
		} else
			HIPCHK(hipMemcpyAsync(d_scratch.get(), prev_scratch, sizeof(float) * (size_t)npl * rp.chunks * 2 * kGroup, hipMemcpyHostToDevice, stream_));
	}
	HIPCHK(hipMemcpyAsync(d_search.get(), searches, sizeof(QSearch) * (size_t)ns, hipMemcpyHostToDevice, stream_));
	for (int s = 0; s < ns; s++)
		if (searches[s].count > 0)
			HIPCHK(hipMemcpyAsync(d_nodes.get() + (size_t)s * kQueueCap, nodes + (size_t)s * kQueueCap * 6, sizeof(QNode) * (size_t)searches[s].count, hipMemcpyHostToDevice, stream_));
	HIPCHK(hipMemcpyAsync(d_ctl.get(), &c, sizeof(QCtl), hipMemcpyHostToDevice, stream_));
	HIPCHK(launch_bnb_queue(d_search.get(), d_nodes.get(), ns, qp, d_prev.get(), d_list.get(), d_ub.get(), d_lb.get(), d_scratch.get(), d_ctl.get(), rp.parity, stream_,
	                        nullptr, parent_search ? d_psearch.get() : nullptr, rp.deep != 0));
	HIPCHK(hipMemcpyAsync(searches, d_search.get(), sizeof(QSearch) * (size_t)ns, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(&c, d_ctl.get(), sizeof(QCtl), hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipMemcpyAsync(listed, d_list.get(), sizeof(ParentRec) * ncap, hipMemcpyDeviceToHost, stream_));
	if (parent_search) HIPCHK(hipMemcpyAsync(parent_search, d_psearch.get(), sizeof(int) * ncap, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	for (int s = 0; s < ns; s++) {
		const int cnt = searches[s].count;
		if (cnt < 0 || cnt > rp.cap) throw std::logic_error("goicp: debug_queue_round: the kernel left a queue longer than cap");
		if (cnt > 0) HIPCHK(hipMemcpy(nodes + (size_t)s * kQueueCap * 6, d_nodes.get() + (size_t)s * kQueueCap, sizeof(QNode) * (size_t)cnt, hipMemcpyDeviceToHost));
	}
	ctl[0] = c.n_groups[0]; ctl[1] = c.n_groups[1]; ctl[2] = c.n_active[0]; ctl[3] = c.n_active[1]; ctl[4] = c.overflow; ctl[5] = c.tile_hint;
}

void Engine::debug_select(const float* d2, size_t n, int num, int kernel, unsigned char* include)
{
	if (n < 1 || n > 0x7fffffffu || num < 1 || (size_t)num > n || kernel < 0 || kernel > 2 || (kernel == 1 && n > 32768))
		throw std::invalid_argument("goicp: debug_select: bad n / num / kernel");
	DeviceGuard guard(dev_);
	Buf<float> dd(n);
	Buf<unsigned char> di(n);
	Buf<IcpState> ds(1);
	HIPCHK(hipMemcpyAsync(dd.get(), d2, sizeof(float) * n, hipMemcpyHostToDevice, stream_));
	HIPCHK(hipMemsetAsync(ds.get(), 0, sizeof(IcpState), stream_));                 // converged = 0
	HIPCHK(hipMemsetAsync(di.get(), 0xff, n, stream_));                             // every flag is written by the kernel
	HIPCHK(launch_icp_select(dd.get(), (int)n, num, ds.get(), di.get(), kernel, stream_));
	HIPCHK(hipMemcpyAsync(include, di.get(), n, hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
}

long long Engine::debug_cache_hits(const float R[9], const float t[3])
{
	// two scoring passes at the same pose: the second one's queries should all hit the neighbour cache
	DeviceGuard guard(dev_);
	if (!d_nn_cache_ || !p_.icp_nn_cache) return -1;
	icp_state_init(R, t, 0.f, 0, 1);
	icp_launch_one();
	HIPCHK(hipMemsetAsync(d_icp_ticket_ + 8, 0, sizeof(int), stream_));
	count_hits_ = true;
	struct Off { bool& b; ~Off() { b = false; } } off{count_hits_};
	icp_launch_one();
	int hits = 0;
	HIPCHK(hipMemcpyAsync(&hits, d_icp_ticket_ + 8, sizeof(int), hipMemcpyDeviceToHost, stream_));
	HIPCHK(hipStreamSynchronize(stream_));
	return hits;
}

void Engine::icp_step()
{
	DeviceGuard guard(dev_);
	// one iteration from the current step pose, fresh means, standard Kabsch (icp_kernel.cu:219-279)
	icp_state_init(stepR_, stepT_, 0.f, 0, 0);
	icp_launch_one();
	icp_state_fetch();
	std::memcpy(stepR_, h_icp_state_->R, sizeof(stepR_));
	std::memcpy(stepT_, h_icp_state_->t, sizeof(stepT_));
	cnt_.icp_iters++;
	std::lock_guard<std::mutex> lk(mtx_);
	std::memcpy(snap_.curR, stepR_, sizeof(stepR_));
	std::memcpy(snap_.curT, stepT_, sizeof(stepT_));
	std::memcpy(snap_.optR, stepR_, sizeof(stepR_));
	std::memcpy(snap_.optT, stepT_, sizeof(stepT_));
	snap_.best_sse = h_icp_state_->err_new;
	snap_.counters = cnt_;
}

// ------------------------------------------------------------------------------------------------
// inner (translation) BnB, batched across searches
// ------------------------------------------------------------------------------------------------
void Engine::ensure_stage(size_t B)
{
	Stage& st = stage_;
	if (!st.ev) st.ev.create(hipEventDisableTiming);
	if (B <= st.cap) return;
	const size_t cap = std::max<size_t>(B, st.cap * 2);
	st.cap = 0;
	st.d_parents.alloc(cap / 8 + 1);
	st.d_ub.alloc(2 * cap);                 // ub[B] | lb[B]: one copy back per round
	st.h_parents.alloc(cap / 8 + 1);
	st.h_ub.alloc(2 * cap);
	st.cap = cap;
}

void Engine::QLane::drop_sort()
{
	sort_keys.reset(); sort_order.reset(); sort_hist.reset(); sort_cen.reset();
	sort = QSort{};
}
void Engine::QLane::drop_tile()
{
	for (int k = 0; k < 2; k++) { tile_parents[k].reset(); tile_segs[k].reset(); }
	tile_ub.reset(); tile_lb.reset(); tile_scratch.reset();
	tile = QTile{};
}

// What a lane derives from the source cloud (ensure_lane; again after set_source): the sorted-round setup with the chunk centroids, the
// round's scratch (sized by the sort's chunks) and the tile list, which exists only while tiles_usable()
void Engine::lane_source_buffers(QLane& L)
{
	const size_t max_groups = (size_t)L.list_cap;
	HIPCHK(hipStreamSynchronize(L.stream));
	L.drop_sort();
	L.d_scratch.reset();
	if (!tiles_usable() && L.tile.ub) L.drop_tile();
	// footprint-ordered items for the large rounds (lean grids, untrimmed, clouds of 4..16 chunks of 4 096 points).  Measured, registration in ms,
	// chunk 2 048 | 3 072 | 4 096 | 6 144 | search order: bunny 34.4 | 33.1 | 33.8 | 34.1 | 36.8 (run-to-run +-0.6); bunny mse 1e-4 280 | 277 | 280 | 276 | 295;
	// synthetic 40 k mse 3e-5 798 | 758 | 714 | 725 | 921; spanner 150 k mse 2e-5 223 | 212 | 206 | 201 | 195 -- above ~64 k points the unsorted
	// launch's large chunks win, so the feature stops there
	// round 4: the cloud is cut into TEN chunks (rounded up to 256 points) rather than into chunks of 4 096 points -- re-swept with the threshold at
	// 256 expansions (tools/sort_threshold_probe.py chunks / chunks2, registration in ms): bunny (30 k) 2 048 | 2 560 | 3 072 | 4 096 points =
	// 32.8 | 31.8-32.4 | 32.5 | 34.3, bunny mse 1e-4 271 | 266 | 267 | 270, synthetic 40 k at mse 3e-5 -- | 770 | 765 | 720 (3 584: 744), every second
	// bunny point (15 k) 1 280 .. 4 096: 26.3-27.4, flat: ten chunks is 3 072 / 4 096 / 1 536 points there
	const int kSortChunkPts = (int)(((N_ + 9) / 10 + 255) / 256 * 256);
	const int sort_chunks = (int)((N_ + kSortChunkPts - 1) / kSortChunkPts);
	if (p_.sort_items && bounds_uses_lean(bounds_dt()) && inliers_ >= (int)N_ && N_ >= 12288 && N_ <= 65536 && sort_chunks >= 4 && sort_chunks <= 16) {
		L.sort_cen.alloc(sort_chunks);
		HIPCHK(launch_chunk_centroids(d_src_, (int)N_, kSortChunkPts, L.sort_cen, L.stream));
		L.sort_keys.alloc(max_groups * sort_chunks);
		L.sort_order.alloc(max_groups * sort_chunks);
		L.sort_hist.alloc(qsort_hist_bytes() / sizeof(unsigned));
		L.sort.cen = L.sort_cen; L.sort.keys = L.sort_keys; L.sort.order = L.sort_order; L.sort.hist = L.sort_hist;
		HIPCHK(hipMemsetAsync(L.sort.hist, 0, qsort_hist_bytes(), L.stream));     // kept zero between uses by the kernels themselves
		// sorted rounds from kSortMinGroups expansions.  Round 3 (512 | 1024 | 2048 | 4096): 35.0 | 34.5 | 33.6 | 37.3 ms.  Re-swept in round 4 with the
		// twin lists and the 4 096-point chunks in place (tools/sort_threshold_probe.py, median of 7): 1 | 128 | 512 | 1024 | 2048 | 4096 | off = 33.8 | 33.3 | 33.5 | 33.6 | 34.4 | 36.6 | 36.3 ms;
		// mse 1e-4 / 3e-5 (0.27 / 6.8 s) flat between 128, 256 and 2048 -- so round 1 of a large batch (230 roots x two passes) is sorted too
		constexpr int kSortMinGroups = 256;
		L.sort.chunk_pts = kSortChunkPts; L.sort.chunks = sort_chunks; L.sort.min_groups = kSortMinGroups;
		L.sort.shift = qsort_shift(dt_.V);           // 16-voxel cells (32-voxel cells: 35.1 ms)
	}
	L.d_scratch.alloc(bounds_queue_scratch_floats((int)max_groups, L.sort.order ? L.sort.chunks : 0));
	if (tiles_usable() && !L.tile.ub) {
		// the second expansion list of a round (LDS-staged DT tiles): same capacity as the direct list
		for (int k = 0; k < 2; k++) {
			L.tile_parents[k].alloc(max_groups);
			L.tile_segs[k].alloc(L.seg_cap);
		}
		L.tile_ub.alloc(max_groups * kGroup);
		L.tile_lb.alloc(max_groups * kGroup);
		L.tile_scratch.alloc(bounds_tile_queue_scratch_floats(L.seg_cap));
		L.tile = QTile{{L.tile_parents[0], L.tile_parents[1]}, {L.tile_segs[0], L.tile_segs[1]}, L.tile_ub, L.tile_lb, L.tile_scratch};
	}
}

void Engine::ensure_lane(int li, size_t nsearch)
{
	QLane& L = ql_[li];
	if (!lane_stream_[li]) make_lane_stream(li);     // lanes 2.. : on first use (a stream costs ~2 ms to create)
	L.stream = lane_stream_[li];
	if (nsearch <= L.cap) return;
	// first use: room for a full round of the outer search (rot_batch parents x 8 children x {ub, lb} pass) -- growing in
	// steps would re-allocate the 196 KB-per-search slabs several times in the first rounds
	size_t cap = std::max<size_t>(L.cap, p_.wide_children ? (size_t)16 * (size_t)std::max(1, p_.rot_batch) : 16);
	while (cap < nsearch) cap *= 2;
	HIPCHK(hipStreamSynchronize(L.stream));
	L.cap = 0;
	L.drop_sort();      // sized by the lists: lane_source_buffers makes them again
	L.drop_tile();
	const size_t max_groups = cap * kQueueRoundPop;          // what the round's lists hold; QParams::kmax keeps (searches running) x (their steps) inside
	L.list_cap = (int)max_groups;
	// segments (<= 64 expansions of one search) of the tile list: every search contributes floor(n / 64) full ones and at most one partial
	L.seg_cap = (int)(max_groups / 64 + cap);
	L.d_search.alloc(cap);
	L.h_search.alloc(cap);
	L.d_nodes.alloc(cap * kQueueCap);          // 196 KB per search; HBM is not the scarce resource here
	for (int k = 0; k < 2; k++) L.d_parents[k].alloc(max_groups);
	for (int k = 0; k < 2; k++) L.d_psearch[k].alloc(max_groups);
	L.d_ub.alloc(max_groups * kGroup);
	L.d_lb.alloc(max_groups * kGroup);
	lane_source_buffers(L);
	if (!L.d_ctl) {
		L.d_ctl.alloc(1);
		L.h_ctl.alloc(1);
		std::memset(L.h_ctl, 0, sizeof(QCtl));
		L.ev_ctl.create(hipEventDisableTiming);
	}
	L.cap = cap;
}

// One round of a lane's device queues, queued on the lane's own stream: the queue kernel (digest the previous round's bounds, select the
// next expansions), then the bound evaluation of what it listed -- the direct list, and the tile list when qp.tile_on.  o.count = false:
// a round that belongs to no search (engine creation, debug_queue_expand) and moves no counter
void Engine::queue_round(QLane& L, int nsearch, const QParams& qp, int parity, int max_groups, const RoundOpts& o)
{
	int* const psearch = o.twins ? L.d_psearch[parity].get() : nullptr;
	HIPCHK(launch_bnb_queue(L.d_search, L.d_nodes, nsearch, qp, L.d_parents[parity ^ 1], L.d_parents[parity], L.d_ub, L.d_lb, L.d_scratch, L.d_ctl, parity, L.stream,
	                        o.tiles ? &L.tile : nullptr, psearch, o.deep));
	if (o.read_ctl) {
		// Everything the host looks at after a chunk -- what the last round listed, how many searches are running, overflow, the tile
		// hint -- is written by THIS kernel; the bound evaluations behind it only fill in the bounds the next queue kernel digests.  So the
		// control block is read back here, ahead of the round's bound evaluation, and the host decides and queues the next chunk
		// while those bounds are being evaluated: the same information at the same point of the search as a read-back after the chunk
		// (identical decisions, identical counts) for a 4 us copy in the stream instead of ~45 us of idle GPU per chunk.  Measured: bunny
		// 33.1-33.6 -> 32.8 ms, skull 6.4 -> 6.3, the rest within the spread.  (From a SIDE stream the copy lost: its blit kernel cannot
		// start while the persistent bound kernels hold every CU -- bunny 33.9 ms, synthetic 40 k mse 3e-5 610 -> 642 ms.)
		HIPCHK(hipMemcpyAsync(L.h_ctl, L.d_ctl, sizeof(QCtl), hipMemcpyDeviceToHost, L.stream));
		HIPCHK(hipEventRecord(L.ev_ctl, L.stream));
	}
	if (o.sorted) HIPCHK(launch_queue_sort(L.d_parents[parity], d_rots_, &L.d_ctl->n_groups[parity], max_groups, L.sort, bounds_dt(), L.stream));
	HIPCHK(launch_bounds_queue(d_src_, (int)N_, bounds_dt(), d_rots_, L.d_parents[parity], &L.d_ctl->n_groups[parity], &L.d_ctl->work[parity][0], &L.d_ctl->chunks, max_groups,
	                           inliers_, L.d_scratch, L.d_ub, L.d_lb, L.stream, o.twins ? L.d_search.get() : nullptr, psearch, o.sorted ? &L.sort : nullptr));
	// the tile list's evaluation behind the direct list's, on the lane's own stream: forking it onto a second stream to run beside it was
	// measured slower (EXPERIMENTS R4.8: the tile and gather kernels take each other's occupancy)
	if (qp.tile_on) HIPCHK(launch_bounds_tile_queue(d_src_, (int)N_, dt_, d_rots_, L.tile, L.d_ctl, parity, L.stream));
	if (!o.count) return;
	cnt_.bounds_launches++;
	queue_rounds_++;
	if (qp.tile_on) tile_rounds_++;
}

// The inner searches with their queues on the device: a round = bnb_queue_kernel (digest the previous round's
// bounds, select the next expansions) + the bound evaluation of the listed expansions; the host queues rounds and
// looks at one word every few rounds.  Same bounds, same stop and prune rules as run_inner_host.
bool Engine::run_inner_device(std::vector<InnerSearch*>& searches, const std::vector<Rot9>& rots)
{
	TraceRange tr("goicp:inner_bnb_rounds");
	const size_t S = searches.size(), nrot = rots.size();
	const int K = std::min(std::max(1, p_.trans_batch), kQueueRoundPop);
	upload_rots(rots);
	// Lanes: the searches of a batch are independent of each other (own queue, own incumbent; only the two passes of one rotation child --
	// twins, same rotation slot -- share loads), so a large batch is cut into lanes by rotation slot and each lane runs its own lock-step rounds
	// on its own stream with its own lists and control block.  Same bounds, same stop and prune rules per search; what changes is that one
	// lane's dependent launches (queue kernel -> sort -> bound evaluation, each draining before the next starts) run beside the others'.
	// That pays when a round is throughput-bound (its kernels' drain tails are what the other lanes fill) and costs when it is latency-bound
	// (the parts of a round take longer than the whole).  Measured (tools/lanes_probe.py; one lane -> two always -> auto with three):
	// rounds of 416 M point-expansions (bunny, mse 3e-5) 6.74 -> 5.71 -> 5.71 s, 183 M (synthetic 40 k, mse 3e-5) 721 -> 669 -> 649 ms, 90 M (bunny,
	// mse 1e-4) 269 -> 264 -> 262 ms, 39 M (3 k points, mse 3e-5) 1.10 -> 1.22 -> 1.02 s (its heavy batches only), 20 M (the default bunny
	// registration) 33.7 -> 34.2 -> 33.1 ms (never cut).  So lanes = 0 (auto) cuts a batch when the PREVIOUS batch's mean round was at least
	// kLaneMinWork point-expansions (swept 16 / 32 / 64 / 128 / 256 M: 64 M) -- a count, not a time: the choice is deterministic
	const bool lanes_wanted = lanes_ >= 2 || (lanes_ == 0 && last_round_work_ >= kLaneMinWork);
	int nl = (lanes_wanted && S >= (size_t)lane_min_searches_) ? std::min(kMaxLanes, lanes_ >= 2 ? lanes_ : kAutoLanes) : 1;
	struct Run {
		QLane* L = nullptr;
		std::vector<int> idx;                 // lane slot -> index into `searches`
		QParams qp{};
		int parity = 0, chunk = 3, rounds_done = 0, last = 0;
		long long round_cap = 0;
		bool sort_round = false, tiles = false, twins = false, done = false;
	} run[kMaxLanes];
	if (nl > 1) {
		for (size_t i = 0; i < S; i++) run[searches[i]->rot_slot % nl].idx.push_back((int)i);
		for (int li = 0; li < nl; li++) if (run[li].idx.empty()) nl = 1;           // (a batch whose slots all fall into one class: not worth a lane)
		if (nl == 1) for (Run& r : run) r.idx.clear();
	}
	if (nl == 1) { run[0].idx.resize(S); for (size_t i = 0; i < S; i++) run[0].idx[i] = (int)i; }
	if (nl > 1) {            // the other lanes start behind the rotation upload (and everything else queued on the engine's stream)
		HIPCHK(hipEventRecord(ev_fork_, stream_));
		for (int li = 1; li < nl; li++) {
			if (!lane_stream_[li]) make_lane_stream(li);     // lanes 2.. : on first use (a stream costs ~2 ms to create)
			HIPCHK(hipStreamWaitEvent(lane_stream_[li], ev_fork_, 0));
		}
	}
	for (int li = 0; li < nl; li++) {
		Run& r = run[li];
		const size_t Sl = r.idx.size();
		ensure_lane(li, Sl);
		QLane& L = ql_[li];
		r.L = &L;
		for (size_t i = 0; i < Sl; i++) {
			const InnerSearch& src = *searches[(size_t)r.idx[i]];
			QSearch& q = L.h_search[i];
			std::memset(&q, 0, sizeof(q));
			q.best = src.best; q.coeff = src.coeff; q.rot = src.rot_slot;
			q.twin = -1;
		}
		// the two searches of a rotation child (same rotation slot, one upper-bound pass with coeff 0, one lower-bound pass): each other's twin
		if (p_.twin_fusion && L.d_psearch[0]) {
			std::vector<int> first(nrot, -1);
			for (size_t i = 0; i < Sl; i++) {
				const int rs = L.h_search[i].rot;
				if (first[(size_t)rs] < 0) { first[(size_t)rs] = (int)i; continue; }
				const int j = first[(size_t)rs];
				if (L.h_search[j].twin < 0 && (L.h_search[j].coeff == 0.f) != (L.h_search[i].coeff == 0.f)) { L.h_search[j].twin = (int)i; L.h_search[i].twin = j; }
			}
		}
		HIPCHK(hipMemcpyAsync(L.d_search, L.h_search, sizeof(QSearch) * Sl, hipMemcpyHostToDevice, L.stream));
		r.qp = queue_params();
		r.qp.list_cap = L.list_cap; r.qp.seg_cap = L.seg_cap;
		r.qp.soft_overflow = 1;
		r.qp.K = K;
		r.qp.kmax = std::min(kQueueMaxPop, L.list_cap / (int)std::max<size_t>(Sl, 1));   // >= kQueueRoundPop: Sl <= the slots the lists were sized for
		HIPCHK(launch_bnb_init(L.d_search, L.d_nodes, (int)Sl, r.qp, L.d_ctl, L.stream));
		// the tile list: always on (lds_tiles 1), or -- the default -- only for the rounds that follow a read-back in which searches
		// qualified (QCtl::tile_hint moved): shallow batches, i.e. every default registration, never pay for the extra launch
		r.tiles = L.tile.ub != nullptr;
		r.twins = p_.twin_fusion && L.d_psearch[0] != nullptr;
		// footprint-ordered items: the sort is queued only for rounds that can reach sort.min_groups expansions -- the first rounds of a
		// batch by what a search can list in them (1, 8, 64 .. nodes), later ones by what the last read-back saw
		r.round_cap = (long long)Sl;
		r.sort_round = L.sort.order != nullptr;
		r.qp.tile_on = r.tiles && (p_.lds_tiles == 1 || (p_.lds_tiles == 2 && tile_sticky_)) ? 1 : 0;
		L.tile_hint_seen = 0;
	}
	// which build of the queue kernel: the batches of a deep run (following one that was fed from tiles: long bound evaluations, queue kernels of several
	// lanes side by side) take the 64-VGPR one (two searches per CU), the others the 128-VGPR one (no spills).  Measured (all-64 -> by batch): skull 6.3 ->
	// 6.17 ms, synthetic 40 k 11.3 -> 11.05 ms, bunny mse 1e-4 260 -> 255 ms, synthetic 40 k mse 3e-5 617 -> 609 ms; all-128: bunny mse 3e-5 5.02 -> 5.18 s
	const bool deep_batch = tile_sticky_;
	// One chunk of rounds of a lane: queue kernel + (sort) + bound evaluation(s) per round; the control block is read back behind the LAST round's queue kernel.
	auto submit = [&](Run& r) {
		ScopedMs t{t_submit_};
		QLane& L = *r.L;
		const size_t Sl = r.idx.size();
		QParams& qp = r.qp;
		const int max_groups = (int)std::min<size_t>(Sl * (size_t)std::min(qp.kmax, 4 * qp.K), (size_t)L.list_cap);   // most the round can list (the kernel widens a stale search's step up to x4)
		RoundOpts o;
		o.tiles = r.tiles; o.twins = r.twins; o.deep = deep_batch;
		for (int k = 0; k < r.chunk; k++) {
			o.read_ctl = k == r.chunk - 1;
			o.sorted = r.sort_round && std::min<long long>(r.round_cap, max_groups) >= L.sort.min_groups;
			queue_round(L, (int)Sl, qp, r.parity, max_groups, o);
			if (r.round_cap < (1ll << 40)) r.round_cap *= 8;
			r.rounds_done++;
			r.last = r.parity;
			r.parity ^= 1;
		}
	};
	// fold a chunk's read-back into the parameters of the chunks still to be queued
	auto adapt = [&](Run& r, const QCtl& c) {
		QLane& L = *r.L;
		QParams& qp = r.qp;
		// (a batch that follows one that used the tile list keeps it on for all of its rounds: an idle tile launch costs a few microseconds, a
		// qualifying search sent through the gather list costs 1.6x per cube bound -- prove-the-optimum bunny 5.18 -> 5.0 s)
		if (r.tiles && p_.lds_tiles == 2) { qp.tile_on = (c.tile_hint != L.tile_hint_seen || tile_sticky_) ? 1 : 0; L.tile_hint_seen = c.tile_hint; }
		// (later rounds of a batch are narrow -- their expansions lie close together whatever the order -- and in long registrations the three
		// extra launches per round are not free on the host side: mse 1e-4 bunny 295 vs 302 ms with the sort queued in every wide round)
		r.sort_round = L.sort.order != nullptr && c.n_groups[r.last] >= L.sort.min_groups && r.rounds_done < 7;
		// the stragglers: when the last round listed few expansions, few searches are still running and the chip is
		// mostly idle -- let each of them expand more nodes per round (fewer latency-bound rounds; the extra speculation
		// costs nothing the chip was using)
		r.chunk = 4;
		// exact: the searches that listed expansions in the last round (a search only ever finishes, so it bounds the rounds to come)
		const int active = std::max(1, c.n_active[r.last]);
		qp.kmax = std::min(kQueueMaxPop, L.list_cap / active);
		if (p_.adaptive_k && K >= 32) {
			// <= 16 running: up to 512 expansions each (swept 1 / 2 / 4 / 8 / 16 searches: the same within the run-to-run spread)
			qp.K = active <= 16 ? kQueueMaxPop : (active <= 64 ? std::min(kQueueRoundPop, 2 * K) : K);
		}
	};
	// lock-step with the host, lane by lane: queue a chunk, wait for it, look at it (a lone lane leaves the GPU idle ~45 us per chunk while
	// the host decides; with two lanes the other lane's chunk is running meanwhile).  Staying a chunk AHEAD of the read-backs instead was
	// built and measured in round 4 (EXPERIMENTS R4.9): the late round width cost more rounds than the bubbles it removed -- removed again.
	bool overflow = false;
	for (int li = 0; li < nl; li++) submit(run[li]);
	for (int live = nl; live > 0;) {
		for (int li = 0; li < nl; li++) {
			Run& r = run[li];
			if (r.done) continue;
			{ ScopedMs t{t_wait_}; HIPCHK(hipEventSynchronize(r.L->ev_ctl)); }
			const QCtl& c = *r.L->h_ctl;
			if (c.overflow) overflow = true;
			if (c.overflow || overflow || (c.n_groups[r.last] == 0 && c.n_tile_groups[r.last] == 0) || cancel_.load()) { r.done = true; live--; continue; }
			adapt(r, c);
			submit(r);
		}
	}
	if (overflow) {
		for (int li = 0; li < nl; li++) HIPCHK(hipStreamSynchronize(run[li].L->stream));
		queue_fallbacks_++; cnt_.queue_fallbacks++;
		return false;
	}
	// the running totals of the whole batch and the searches' results in one round trip per lane
	const double t2 = now_ms();
	for (int li = 0; li < nl; li++) {
		QLane& L = *run[li].L;
		HIPCHK(hipMemcpyAsync(L.h_ctl, L.d_ctl, sizeof(QCtl), hipMemcpyDeviceToHost, L.stream));
		HIPCHK(hipMemcpyAsync(L.h_search, L.d_search, sizeof(QSearch) * run[li].idx.size(), hipMemcpyDeviceToHost, L.stream));
	}
	for (int li = 0; li < nl; li++) HIPCHK(hipStreamSynchronize(run[li].L->stream));
	for (int li = 0; li < nl; li++) if (run[li].L->h_ctl->overflow) overflow = true;
	if (overflow) { queue_fallbacks_++; cnt_.queue_fallbacks++; return false; }
	if (nl > 1) cnt_.lane_batches++;
	long long cubes = 0, tile_total = 0;
	int rounds = 1;
	for (int li = 0; li < nl; li++) {
		tile_total += run[li].L->h_ctl->tile_total;
		rounds = std::max(rounds, run[li].rounds_done);
		for (size_t i = 0; i < run[li].idx.size(); i++) cubes += run[li].L->h_search[i].cubes;
	}
	last_round_work_ = (double)cubes / kGroup / rounds * (double)N_;
	tile_sticky_ = tile_total > 0 && (double)tile_total * kGroup >= kTileStickyShare * (double)cubes;
	for (int li = 0; li < nl; li++) {
		const QLane& L = *run[li].L;
		cnt_.tile_expansions += L.h_ctl->tile_total;
		if (p_.verbose) for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) sel_hist_[a][b] += L.h_ctl->sel_hist[a][b];
		for (size_t i = 0; i < run[li].idx.size(); i++) {
			const QSearch& q = L.h_search[i];
			InnerSearch& s = *searches[(size_t)run[li].idx[i]];
			if (q.done == 2) { redo_.push_back(&s); continue; }          // its queue outgrew the slab: untouched here, re-run by run_inner through the host queues
			s.finish(SearchOut::of(q));
		}
	}
	t_collect_ += now_ms() - t2;
	return true;
}

void Engine::run_inner(std::vector<InnerSearch*>& searches, const std::vector<Rot9>& rots)
{
	DeviceGuard guard(dev_);
	for (auto* s : searches)
		if (s->rot_slot < 0 || (size_t)s->rot_slot >= rots.size()) throw std::logic_error("goicp: rotation slot out of range");
	if (p_.device_queues && p_.trans_batch > 1) {
		redo_.clear();
		bool ok;
		{ ScopedMs t{bnb_ms_}; ok = run_inner_device(searches, rots); }
		if (ok && redo_.empty()) return;
		if (ok) {
			// searches whose queue outgrew its slab (they have not been touched): through the host queues, alone
			queue_fallbacks_++; cnt_.queue_fallbacks++;
			std::vector<InnerSearch*> redo;
			redo.swap(redo_);
			run_inner_host(redo, rots, true);
			return;
		}
		// a round's lists overflowed: the whole batch is re-run through the host queues (the searches have not been touched)
		run_inner_host(searches, rots, true);
		return;
	}
	run_inner_host(searches, rots);
}

// Lock-step rounds of all the given inner searches: pop up to trans_batch nodes per search, evaluate the
// 8 children of every popped node in ONE launch, digest the bounds, repeat until every search stops.
// fallback (a device queue outgrew its slab -- a search with tens of thousands of queued nodes): the round of a search whose
// incumbent did not improve in its last round grows x4, then x16 (the stale-incumbent rule of the device queues: a search that
// is proving expands every node with best - lb >= SSEThresh whatever the order, and the host's heap has no 128-node limit), so
// the re-run is a few hundred large launches instead of thousands of small ones
void Engine::run_inner_host(std::vector<InnerSearch*>& searches, const std::vector<Rot9>& rots, bool fallback)
{
	DeviceGuard guard(dev_);
	ScopedMs acc{bnb_ms_};
	const int K0 = std::max(1, p_.trans_batch);
	const bool widen = fallback && p_.adaptive_k && p_.stale_widen && K0 > 1;
	upload_rots(rots);
	Stage& st = stage_;

	// One group per round.  (Measured on MI355X: splitting the searches into two alternating groups so
	// that the host digests one group's results while the GPU evaluates the other's did not pay --
	// 0.087 s vs 0.083 s on the full bunny: the rounds are bound by the small launches themselves, not by
	// host work.)
	auto submit = [&]() -> bool {
		ScopedMs t{t_submit_};
		size_t B = 0;
		for (auto* s : searches) {
			s->parents.clear();
			if (s->done) continue;
			const int K = !widen ? K0 : (s->stale >= 3 ? 16 * K0 : (s->stale >= 1 ? 4 * K0 : K0));
			while ((int)s->parents.size() < K && !s->pq.empty()) {
				const Node n = s->pq.top();
				if (s->best - n.lb < sse_thresh_) {           // jly_goicp.cpp:257
					if (s->parents.empty()) { s->pq.pop(); s->pops++; s->done = true; }
					break;
				}
				s->pq.pop();
				s->pops++;
				s->parents.push_back(n);
			}
			if (s->parents.empty()) { s->done = true; continue; }
			B += 8 * s->parents.size();
		}
		if (B == 0) return false;
		ensure_stage(B);
		size_t o = 0;
		for (auto* s : searches)
			for (const Node& par : s->parents) {
				// the kernels expand the 8 children themselves (load_group in device.hip; jly_goicp.cpp:262-273)
				ParentRec& r = st.h_parents[o++];
				if (p_.verbose) { int lv = 0; for (float w = par.w; w < trans_root_.w && lv < 31; w *= 2) lv++; level_hist_[lv]++; }
				r.x = par.x; r.y = par.y; r.z = par.z; r.w = par.w; r.coeff = s->coeff; r.rot = s->rot_slot;
			}
		st.B = B;
		HIPCHK(hipMemcpyAsync(st.d_parents, st.h_parents, sizeof(ParentRec) * (B / 8), hipMemcpyHostToDevice, stream_));
		eval_bounds_dev(d_rots_, nullptr, (int)B, st.d_ub, st.d_ub + B, stream_, st.d_parents);
		HIPCHK(hipMemcpyAsync(st.h_ub, st.d_ub, sizeof(float) * 2 * B, hipMemcpyDeviceToHost, stream_));
		HIPCHK(hipEventRecord(st.ev, stream_));
		return true;
	};
	auto collect = [&] {
		ScopedMs t{t_collect_};
		size_t o = 0;
		for (auto* s : searches) {
			const float best_before = s->best;
			for (const Node& par : s->parents)
				for (int j = 0; j < 8; j++, o++) {
					Node c = child_cube(par, j);
					const float ub = st.h_ub[o], lb = st.h_ub[st.B + o];
					s->cubes++;
					if (trans_boxed_ && !in_box(c, trans_lo_, trans_hi_)) continue;   // outside the configured translation range
					if (ub < s->min_ub) s->min_ub = ub;
					if (ub < s->best) { s->best = ub; s->best_node = c; s->improved = true; }   // :319-324
					if (lb >= s->best) continue;                                                  // :327
					if (p_.trans_search_depth > 0 && !(std::ldexp(c.w, p_.trans_search_depth) > trans_root_.w)) continue;   // depth limit reached: evaluated, not expanded
					c.ub = ub; c.lb = lb;
					s->pq.push(c);
				}
			if (!s->parents.empty()) s->stale = s->best < best_before ? 0 : s->stale + 1;
		}
	};
	while (submit()) {
		{ ScopedMs t{t_wait_}; HIPCHK(hipEventSynchronize(st.ev)); }
		collect();
		if (cancel_.load()) break;
	}
	HIPCHK(hipStreamSynchronize(stream_));
}

float Engine::inner_bnb(const float R[9], int level, float incumbent, float best_node[4], Counters* c)
{
	DeviceGuard guard(dev_);
	std::vector<Rot9> rots(1);
	std::memcpy(rots[0].r, R, sizeof(float) * 9);
	InnerSearch s = fresh_search(0, rot_coeff(level), incumbent);
	std::vector<InnerSearch*> v{&s};
	run_inner(v, rots);
	if (best_node && s.improved) { best_node[0] = s.best_node.x; best_node[1] = s.best_node.y; best_node[2] = s.best_node.z; best_node[3] = s.best_node.w; }
	cnt_.trans_pops += s.pops; cnt_.cubes += s.cubes; cnt_.inner_calls++;
	if (c) { c->trans_pops += s.pops; c->cubes += s.cubes; c->inner_calls++; c->queue_fallbacks = cnt_.queue_fallbacks; }
	return s.best;
}

// ------------------------------------------------------------------------------------------------
// outer (rotation) BnB
// ------------------------------------------------------------------------------------------------
void Engine::publish(bool finished)
{
	Result copy;
	{
		std::lock_guard<std::mutex> lk(mtx_);
		std::memcpy(snap_.optR, optR_, sizeof(optR_)); std::memcpy(snap_.optT, optT_, sizeof(optT_));
		std::memcpy(snap_.curR, curR_, sizeof(curR_)); std::memcpy(snap_.curT, curT_, sizeof(curT_));
		snap_.best_sse = opt_err_;
		snap_.finished = finished ? 1 : 0;
		snap_.counters = cnt_;
		snap_.dt_build_ms = dt_build_ms_;
		snap_.register_ms = register_ms_;
		copy = snap_;
	}
	if (progress_cb_) progress_cb_(copy);      // outside the lock: the callback may poll
}

Result Engine::poll()
{
	std::lock_guard<std::mutex> lk(mtx_);
	return snap_;
}

void Engine::adopt(float err, const float R[9], const float t[3])
{
	opt_err_ = err;
	std::memcpy(optR_, R, sizeof(optR_));
	std::memcpy(optT_, t, sizeof(optT_));
}

float Engine::icp_from(float R[9], float t[3])
{
	TraceRange tr("goicp:icp_run+rescore");
	ScopedMs acc{icp_ms_};
	// GoICP::ICP (jly_goicp.cpp:93-132): ICP3D::Run, then re-score with the DT
	int it = 0;
	if (icp_comm_) {
		float ei = 0.f;
		const int rc = icp_run_collective(icp_comm_, R, t, p_.icp_max_iter, icp_err_diff_, &ei, &it);
		if (rc != GOICP_OK) throw StatusError(rc, "collective ICP failed (status " + std::to_string(rc) + ")");
	} else {
		icp_run(R, t, p_.icp_max_iter, icp_err_diff_, &it);
	}
	const float e = eval_sse(R, t);
	if (p_.verbose > 1) std::fprintf(stderr, "[goicp] ICP run: %d iterations, %.2f ms, error %.6g (rot pops so far %lld, cube bounds %lld)\n", it, now_ms() - acc.t0, e, cnt_.rot_pops, cnt_.cubes);
	return e;
}

void Engine::offer_global_best(float sse, const float R[9], const float t[3])
{
	DeviceGuard guard(dev_);
	if (sse < opt_err_) {
		adopt(sse, R, t);
		unrefined_ = false;          // the collective protocol offers refined poses only
		prune_queue();
		if (opt_err_ < sse_thresh_) early_exit_ = true;
		publish(false);
	}
}

void Engine::prune_queue()
{
	std::priority_queue<Node> nq;
	while (!queue_.empty()) {
		Node n = queue_.top(); queue_.pop();
		if (n.lb < opt_err_) nq.push(n); else break;
	}
	queue_.swap(nq);
}

void Engine::register_begin()
{
	DeviceGuard guard(dev_);
	registering_.store(1);
	cancel_.store(false);
	early_exit_ = converged_ = false;
	rot_ramp_ = 8;
	unrefined_ = false;
	last_round_work_ = 0; tile_sticky_ = false;      // every registration starts single-lane (determinism: the choice depends on this registration only)
	icp_ms_ = 0; t_submit_ = t_wait_ = t_collect_ = 0;
	std::memset(level_hist_, 0, sizeof(level_hist_));
	cnt_ = Counters{};
	while (!queue_.empty()) queue_.pop();
	if (flow_mode()) { ensure_lane(0, kFlowSearches); flow_reset(); }
	const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	const float Z[3] = {0, 0, 0};
	// initial error (jly_goicp.cpp:357-372) and initial ICP (:375-391)
	opt_err_ = eval_sse(I, Z);
	std::memcpy(optR_, I, sizeof(I)); std::memcpy(optT_, Z, sizeof(Z));
	float R[9], t[3];
	std::memcpy(R, I, sizeof(I)); std::memcpy(t, Z, sizeof(Z));
	float e = icp_from(R, t);
	if (e < opt_err_) adopt(e, R, t);
	std::memcpy(curR_, optR_, sizeof(optR_)); std::memcpy(curT_, optT_, sizeof(optT_));
	if (p_.verbose) std::fprintf(stderr, "[goicp] init error %.6g (after ICP)\n", opt_err_);
	bnb_ms_ = 0;

	const Node root = rot_root_;   // jly_goicp.cpp:44-48 unless [params.rotation] narrows it
	if (world_ <= 1) {
		queue_.push(root);
	} else {
		// shard: expand the root two levels (64 cubes) and deal them round-robin to the ranks; the
		// parents' bounds are 0, so nothing is lost
		int k = 0;
		for (int a = 0; a < 8; a++) {
			const Node c1 = child_cube(root, a);
			for (int b = 0; b < 8; b++, k++) {
				Node c2 = child_cube(c1, b);
				c2.l = 2;
				if (rot_boxed_ && !in_box(c2, rot_lo_, rot_hi_)) continue;
				if (k % world_ == rank_) queue_.push(c2);
			}
		}
	}
	publish(false);
}

// the rotation children of the given parents that survive the pi-ball and range culls (jly_goicp.cpp:427-467)
void Engine::make_kids(const std::vector<Node>& parents, std::vector<Kid>& kids)
{
	for (const Node& parent : parents) {
		for (int j = 0; j < 8; j++) {
			Node c = child_cube(parent, j);          // jly_goicp.cpp:427-428
			c.l = parent.l + 1;
			float v1 = c.x + c.w / 2, v2 = c.y + c.w / 2, v3 = c.z + c.w / 2;
			// pi-ball cull (:443): float sqrt, double subtraction and comparison
			if ((double)std::sqrt(v1 * v1 + v2 * v2 + v3 * v3) - kSQRT3 * (double)c.w / 2 > kPI) continue;
			if (rot_boxed_ && !in_box(c, rot_lo_, rot_hi_)) continue;     // outside the configured rotation range
			Kid k;
			k.node = c;
			k.parent_lb = parent.lb;
			rodrigues(v1, v2, v3, k.R);
			kids.push_back(k);
		}
	}
}

// jly_goicp.cpp:495-544: the upper-bound search of a rotation child is in; returns true on the early exit (:527)
bool Engine::handle_ub(Kid& k, const SearchOut& s)
{
	cnt_.trans_pops += s.pops; cnt_.cubes += s.cubes; cnt_.inner_calls++;
	k.node.ub = s.best;
	// the widened search orders rotation cubes of equal lower bound (all the shallow ones: lb = 0) by the smallest upper bound
	// their own upper-bound search saw -- the basin most likely to refine the optimum is expanded first.  The reference leaves
	// that order to its heap (any order of a best-first BnB is valid); the reference-order mode keeps the key at 0.
	k.node.tie = (p_.wide_children && p_.ub_tiebreak && std::isfinite(s.min_ub)) ? s.min_ub : 0.f;
	std::memcpy(curR_, k.R, sizeof(curR_));
	if (s.improved) { curT_[0] = s.best_node.x + s.best_node.w / 2; curT_[1] = s.best_node.y + s.best_node.w / 2; curT_[2] = s.best_node.z + s.best_node.w / 2; }
	if (!(s.best < opt_err_) || !s.improved) return false;
	float t[3] = {s.best_node.x + s.best_node.w / 2, s.best_node.y + s.best_node.w / 2, s.best_node.z + s.best_node.w / 2};
	adopt(s.best, k.R, t);
	if (icp_comm_) {
		// collective refinement (goicp_register_sharded_collective_icp): the upper bound is adopted as it is; the protocol refines the
		// global winner on every rank after the next exchange, so no pose is refined twice
		unrefined_ = true;
		publish(false);
		if (opt_err_ < sse_thresh_) { early_exit_ = true; return true; }
		prune_queue();
		return false;
	}
	float R[9], ti[3];
	std::memcpy(R, k.R, sizeof(R)); std::memcpy(ti, t, sizeof(ti));
	float e = icp_from(R, ti);
	if (e < opt_err_) adopt(e, R, ti);
	if (p_.verbose) std::fprintf(stderr, "[goicp] rank %d  error* %.6g (ub %.6g, level %d)\n", rank_, opt_err_, s.best, k.node.l);
	publish(false);
	if (opt_err_ < sse_thresh_) { early_exit_ = true; return true; }   // :527
	prune_queue();                                                      // :533-543
	return false;
}

// :551-562: the lower-bound search is in
void Engine::handle_lb(Kid& k, const SearchOut& s)
{
	cnt_.trans_pops += s.pops; cnt_.cubes += s.cubes; cnt_.inner_calls++;
	if (s.best >= opt_err_) return;
	if (p_.rot_search_depth > 0 && k.node.l >= p_.rot_search_depth) return;   // depth limit: evaluated, not expanded
	k.node.lb = s.best;
	queue_.push(k.node);
}

void Engine::process_parents(const std::vector<Node>& parents)
{
	TraceRange tr("goicp:rotation_batch");
	std::vector<Kid> kids;
	make_kids(parents, kids);
	if (kids.empty()) return;
	std::vector<Rot9> rots(kids.size());
	for (size_t i = 0; i < kids.size(); i++) std::memcpy(rots[i].r, kids[i].R, sizeof(float) * 9);

	if (p_.wide_children) {
		// every child's upper-bound AND lower-bound search in lock-step: one launch per round covers
		// up to 16 searches per rotation parent.  The searches start from the incumbent of the batch
		// start (the reference lets earlier children tighten it: fewer nodes, same bounds).
		std::vector<InnerSearch> ubs, lbs;
		ubs.reserve(kids.size()); lbs.reserve(kids.size());
		for (size_t i = 0; i < kids.size(); i++) { ubs.push_back(fresh_search((int)i, 0.f, opt_err_)); lbs.push_back(fresh_search((int)i, rot_coeff(kids[i].node.l), opt_err_)); }
		std::vector<InnerSearch*> ptr;
		// a child's two searches side by side: they share the rotation, expand the same root and a third of the same
		// depth-1 nodes in the same rounds, and the bound kernel walks the expansions in search order -- the second of the
		// pair finds the first one's DT lines in L2 (shallow rounds are bound by compulsory line fetches)
		for (size_t i = 0; i < kids.size(); i++) { ptr.push_back(&ubs[i]); ptr.push_back(&lbs[i]); }
		run_inner(ptr, rots);
		for (size_t i = 0; i < kids.size(); i++) {
			if (handle_ub(kids[i], SearchOut::of(ubs[i]))) return;
			handle_lb(kids[i], SearchOut::of(lbs[i]));
		}
	} else {
		for (size_t i = 0; i < kids.size(); i++) {
			InnerSearch u = fresh_search((int)i, 0.f, opt_err_);
			std::vector<InnerSearch*> p1{&u};
			run_inner(p1, rots);
			if (handle_ub(kids[i], SearchOut::of(u))) return;
			InnerSearch l = fresh_search((int)i, rot_coeff(kids[i].node.l), opt_err_);
			std::vector<InnerSearch*> p2{&l};
			run_inner(p2, rots);
			handle_lb(kids[i], SearchOut::of(l));
			if (cancel_.load()) return;
		}
	}
}

// ------------------------------------------------------------------------------------------------
// Continuous flow (wide mode + device-resident queues): rotation children are admitted in batches but HARVESTED one by
// one -- a child is handled as soon as both its searches have stopped, its slots are recycled, and the next batch of
// parents is admitted when the number of running searches falls below a low-water mark, instead of waiting for the
// slowest search of the batch.  (Lock-step batches ended in ~5 rounds with a handful of active searches each, at the
// latency floor of three launches; those rounds now carry the next batch's work.)  Any expansion order of a best-first BnB
// is valid; the searches of a child start from the incumbent at its admission.
// ------------------------------------------------------------------------------------------------
void Engine::flow_reset()
{
	flights_.clear();
	free_search_.clear(); free_rot_.clear();
	for (int i = kFlowSearches - 1; i >= 0; i--) free_search_.push_back(i);
	for (int i = kFlowSearches / 2 - 1; i >= 0; i--) free_rot_.push_back(i);
	q_hi_ = 0; q_parity_ = 0; flow_active_ = 0;
	if (ql_[0].d_ctl) HIPCHK(hipMemsetAsync(ql_[0].d_ctl, 0, sizeof(QCtl), stream_));
	// a slot abandoned in flight (early exit, cancel) must not come back as a live search: an all-zero record is an empty
	// queue that marks itself done at first touch
	if (ql_[0].d_search) HIPCHK(hipMemsetAsync(ql_[0].d_search, 0, sizeof(QSearch) * ql_[0].cap, stream_));
}

bool Engine::tiles_usable() const
{
	// the tile kernel stages 4x4x4 fp32 bricks and sums every point (no trimming)
	return p_.lds_tiles != 0 && dt_.layout == 1 && !p_.bounds_fp16 && inliers_ >= (int)N_;
}

QParams Engine::queue_params() const
{
	QParams qp{};
	qp.tile_on = 0; qp.tile_min = std::max(8, p_.tile_min);
	qp.tile_spread = tiles_usable() ? (float)((double)p_.tile_spread_vox / dt_.scale) : 0.f;
	qp.tile_stats = p_.verbose ? 1 : 0; qp.tile_stats_scale = (float)dt_.scale;
	qp.stale_widen = p_.adaptive_k ? p_.stale_widen : 0;
	qp.stale_compact = p_.adaptive_k && p_.stale_widen ? p_.stale_compact : 0;

	qp.thr = sse_thresh_; qp.K = std::min(std::max(1, p_.trans_batch), kQueueRoundPop);
	qp.kmax = kQueueRoundPop; qp.list_cap = ql_[0].list_cap; qp.seg_cap = ql_[0].seg_cap;     // any number of searches fits; run_inner_device raises kmax for the last few
	qp.root_x = trans_root_.x; qp.root_y = trans_root_.y; qp.root_z = trans_root_.z; qp.root_w = trans_root_.w;
	qp.boxed = trans_boxed_ ? 1 : 0; qp.depth = p_.trans_search_depth;
	qp.cap = (p_.queue_cap > 0 && p_.queue_cap < kQueueCap) ? p_.queue_cap : kQueueCap;
	for (int k = 0; k < 3; k++) { qp.lo[k] = trans_boxed_ ? trans_lo_[k] : 0.f; qp.hi[k] = trans_boxed_ ? trans_hi_[k] : 0.f; }
	return qp;
}

// a queue outgrew its slab: every child still in flight is finished through the host queues (from its own incumbent)
void Engine::flow_fallback()
{
	queue_fallbacks_++; cnt_.queue_fallbacks++;
	std::vector<Flight> todo;
	for (const Flight& f : flights_) if (!f.handled) todo.push_back(f);
	flow_reset();
	for (Flight& f : todo) {
		std::vector<Rot9> rots(1);
		std::memcpy(rots[0].r, f.kid.R, sizeof(float) * 9);
		InnerSearch u = fresh_search(0, 0.f, f.incumbent), l = fresh_search(0, rot_coeff(f.kid.node.l), f.incumbent);
		std::vector<InnerSearch*> ptr{&u, &l};
		run_inner_host(ptr, rots, true);
		if (handle_ub(f.kid, SearchOut::of(u))) return;
		handle_lb(f.kid, SearchOut::of(l));
	}
}

int Engine::flow_step(int max_rot_pops)
{
	TraceRange tr("goicp:flow_step");
	ScopedMs acc{bnb_ms_};
	const QParams qp = queue_params();
	QLane& L = ql_[0];                // the flow's one lane; its stream is stream_ (ensure_lane)
	ensure_batch(1, kFlowSearches / 2);
	if (!h_qinit_) {
		h_qinit_.alloc(kFlowSearches);
		d_qinit_.alloc(kFlowSearches);
	}
	int pops = 0;
	auto unhandled = [&] { size_t n = 0; for (const Flight& f : flights_) n += f.handled ? 0 : 1; return n; };
	while (!early_exit_ && !cancel_.load()) {
		// ---- admit the next batch of rotation parents when the running searches are few ----
		// at most kFlowSearches / 16 parents per admission: a batch needs 16 search slots per parent, and with a larger P the
		// admission test below could never pass even with every slot free (rot_batch > 128: the loop would spin forever)
		const int P = std::max(1, std::min(std::min(p_.rot_batch, rot_ramp_), kFlowSearches / 16));
		if (!converged_ && !queue_.empty() && pops < max_rot_pops && flow_active_ <= (flights_.empty() ? kFlowSearches : p_.flow) &&
		    free_search_.size() >= (size_t)16 * P && free_rot_.size() >= (size_t)8 * P) {
			const std::vector<Node> parents = pop_parents(P, max_rot_pops, pops, unhandled() == 0);   // the stop rule is only final once nothing is in flight
			if (!parents.empty()) {
				rot_ramp_ = std::min(rot_ramp_ * 2, 1 << 20);
				std::vector<Kid> kids;
				make_kids(parents, kids);
				int n = 0;
				for (Kid& k : kids) {
					Flight f{};
					f.kid = k; f.incumbent = opt_err_; f.handled = false;
					f.rot_slot = free_rot_.back(); free_rot_.pop_back();
					f.s_ub = free_search_.back(); free_search_.pop_back();
					f.s_lb = free_search_.back(); free_search_.pop_back();
					std::memcpy(h_rots_[f.rot_slot].r, k.R, sizeof(float) * 9);
					h_qinit_[n++] = QInit{f.s_ub, opt_err_, 0.f, f.rot_slot, -1};
					h_qinit_[n++] = QInit{f.s_lb, opt_err_, rot_coeff(k.node.l), f.rot_slot, -1};
					q_hi_ = std::max(q_hi_, std::max(f.s_ub, f.s_lb) + 1);
					flights_.push_back(f);
				}
				if (n) {
					HIPCHK(hipMemcpyAsync(d_rots_, h_rots_, sizeof(Rot9) * (kFlowSearches / 2), hipMemcpyHostToDevice, stream_));
					HIPCHK(hipMemcpyAsync(d_qinit_, h_qinit_, sizeof(QInit) * n, hipMemcpyHostToDevice, stream_));
					HIPCHK(launch_bnb_init_list(L.d_search, L.d_nodes, d_qinit_, n, qp, stream_));
					flow_active_ += n;
				}
			}
		}
		if (unhandled() == 0) break;
		// ---- a chunk of rounds over every slot in use ----
		const double t0 = now_ms();
		QParams qr = qp;
		if (p_.adaptive_k && qp.K >= 32) qr.K = flow_active_ <= 16 ? kQueueRoundPop : (flow_active_ <= 64 ? std::min(kQueueRoundPop, 2 * qp.K) : qp.K);
		// most the round can list: the queue kernel widens a stale search's step up to x4 (stale_widen), as in run_inner_device --
		// sizing the evaluation's grid by q_hi_ * K left the expansions listed beyond it unevaluated in trimmed runs (one workgroup each)
		const int max_groups = (int)std::min<size_t>((size_t)q_hi_ * (size_t)std::min(qr.kmax, 4 * qr.K), (size_t)L.list_cap);
		for (int r = 0; r < 3; r++, q_parity_ ^= 1) queue_round(L, q_hi_, qr, q_parity_, max_groups, RoundOpts{});
		HIPCHK(hipMemcpyAsync(L.h_ctl, L.d_ctl, sizeof(QCtl), hipMemcpyDeviceToHost, stream_));
		HIPCHK(hipMemcpyAsync(L.h_search, L.d_search, sizeof(QSearch) * (size_t)q_hi_, hipMemcpyDeviceToHost, stream_));
		t_submit_ += now_ms() - t0;
		{ ScopedMs t{t_wait_}; HIPCHK(hipStreamSynchronize(stream_)); }
		if (L.h_ctl->overflow) { flow_fallback(); continue; }
		// ---- harvest: every child whose two searches have stopped, in admission order ----
		const double t2 = now_ms();
		int active = 0;
		bool stop = false;
		for (Flight& f : flights_) {
			if (f.handled) continue;
			const QSearch& u = L.h_search[f.s_ub];
			const QSearch& l = L.h_search[f.s_lb];
			// a search that has stopped has no pending children: done is only set in the selection phase, after the digest
			if (!u.done || !l.done) { active += (u.done ? 0 : 1) + (l.done ? 0 : 1); continue; }
			f.handled = true;
			free_search_.push_back(f.s_ub); free_search_.push_back(f.s_lb); free_rot_.push_back(f.rot_slot);
			if (stop) continue;                                                  // early exit taken: the rest is abandoned
			if (handle_ub(f.kid, SearchOut::of(u))) { stop = true; continue; }
			handle_lb(f.kid, SearchOut::of(l));
		}
		t_collect_ += now_ms() - t2;
		flow_active_ = active;
		flights_.erase(std::remove_if(flights_.begin(), flights_.end(), [](const Flight& f) { return f.handled; }), flights_.end());
		if (flights_.empty()) q_hi_ = 0;
		publish(false);
		if (pops >= max_rot_pops && flights_.empty()) break;
	}
	return pops;
}

std::vector<Node> Engine::pop_parents(int P, int max_rot_pops, int& pops, bool may_converge)
{
	std::vector<Node> parents;
	while ((int)parents.size() < P && !queue_.empty() && pops < max_rot_pops) {
		const Node parent = queue_.top();
		if ((opt_err_ - parent.lb) <= sse_thresh_) {      // jly_goicp.cpp:416
			// single rank: global convergence.  sharded: this rank's frontier can no longer improve
			if (parents.empty() && may_converge) { queue_.pop(); cnt_.rot_pops++; pops++; converged_ = true; }
			break;
		}
		queue_.pop();
		cnt_.rot_pops++;
		pops++;
		parents.push_back(parent);
	}
	return parents;
}

StepStatus Engine::register_step(int max_rot_pops)
{
	DeviceGuard guard(dev_);
	int pops = 0;
	if (flow_mode()) {
		const double icp0 = icp_ms_;
		pops = flow_step(max_rot_pops);
		bnb_ms_ -= icp_ms_ - icp0;           // flow_step's clock also ran through the ICP runs it triggered
		publish(false);
	} else
	while (true) {
		if (early_exit_ || cancel_.load() || pops >= max_rot_pops) break;
		if (converged_ || queue_.empty()) break;
		// Rotation parents expanded together: ramps 8, 16, 32 ... rot_batch.  Easy registrations end in
		// the first rounds and pay for little speculation; long searches run with few, large launches
		// (full bunny: 310 launches / 63 ms at a fixed 8, 52 launches / 55 ms at 64).
		const int P = p_.wide_children ? std::max(1, std::min(p_.rot_batch, rot_ramp_)) : 1;
		rot_ramp_ = std::min(rot_ramp_ * 2, 1 << 20);
		std::vector<Node> parents = pop_parents(P, max_rot_pops, pops, true);
		if (parents.empty()) break;
		// ub_share: part of a batch goes to the queued cubes with the smallest upper bound seen inside them, whatever their lower
		// bound -- the early exit (jly_goicp.cpp:527) needs a pose below SSEThresh, and that is found by refining a promising
		// basin, not by closing the gap.  Valid: any expansion order keeps the bounds; the batch's first parents are still the
		// smallest lower bounds, so the stop rule (:416) sees the same frontier.
		if (p_.wide_children && p_.ub_share > 0.f && !converged_ && queue_.size() > 1 && pops < max_rot_pops) {
			size_t want = std::min<size_t>({(size_t)((float)P * p_.ub_share), queue_.size(), (size_t)(max_rot_pops - pops)});
			if (want > 0) {
				std::vector<Node> rest;
				rest.reserve(queue_.size());
				while (!queue_.empty()) { rest.push_back(queue_.top()); queue_.pop(); }
				std::partial_sort(rest.begin(), rest.begin() + (long)want, rest.end(), [](const Node& a, const Node& b) { return a.tie < b.tie; });
				for (size_t i = 0; i < want; i++) { parents.push_back(rest[i]); cnt_.rot_pops++; pops++; }
				for (size_t i = want; i < rest.size(); i++) queue_.push(rest[i]);
			}
		}
		process_parents(parents);
		publish(false);
	}
	StepStatus st{};
	st.early_exit = early_exit_ ? 1 : 0;
	st.finished = (early_exit_ || converged_ || (queue_.empty() && flights_.empty()) || cancel_.load()) ? 1 : 0;
	st.best_sse = opt_err_;
	st.frontier_lb = (queue_.empty() || converged_ || early_exit_) ? std::numeric_limits<float>::infinity() : queue_.top().lb;
	if (!converged_ && !early_exit_)
		for (const Flight& f : flights_) st.frontier_lb = std::min(st.frontier_lb, f.kid.parent_lb);   // children still in flight stand for their parents
	st.rot_pops = cnt_.rot_pops;
	// a step that neither popped a rotation node nor has searches in flight, with work still queued, would make every
	// caller loop (Engine::run, run_sharded) spin forever with the GPU idle: report it instead
	if (!st.finished && pops == 0 && flights_.empty()) throw std::logic_error("goicp: register_step made no progress with a non-empty rotation queue");
	return st;
}

int Engine::donate(int max_nodes, float* out)
{
	// every second cube in priority order leaves (at most max_nodes, never the whole queue): both sides keep
	// cubes of every priority, and the frontier's minimum lower bound stays with the donor
	std::vector<Node> all;
	all.reserve(queue_.size());
	while (!queue_.empty()) { all.push_back(queue_.top()); queue_.pop(); }
	int n = 0;
	for (size_t i = 0; i < all.size(); i++) {
		if ((i & 1) && n < max_nodes) {
			const Node& c = all[i];
			float* o = out + 7 * n++;
			o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w; o[4] = c.tie; o[5] = c.lb; o[6] = (float)c.l;
		} else queue_.push(all[i]);
	}
	return n;
}

void Engine::receive(const float* in, int n)
{
	for (int i = 0; i < n; i++) {
		const float* o = in + 7 * i;
		Node c{o[0], o[1], o[2], o[3], o[4], o[5], (int)o[6]};
		c.tie = o[4];                       // the ub slot of a travelling cube carries its tie-break key
		if (c.lb < opt_err_) queue_.push(c);
	}
	if (!queue_.empty() && !early_exit_) converged_ = false;
	publish(false);
}

void Engine::register_end()
{
	publish(true);
	registering_.store(0);
}

void Engine::run()
{
	DeviceGuard guard(dev_);
	TraceRange tr("goicp:register");
	struct Idle { std::atomic<int>& r; ~Idle() { r.store(0); } } idle{registering_};   // also when the registration throws
	double t0 = now_ms();
	register_begin();
	while (true) {
		StepStatus st = register_step(flow_mode() ? (1 << 20) : std::max(64, p_.rot_batch));     // one batch per step at full ramp (the flow drains its in-flight searches at the end of a step)
		if (st.finished) break;
	}
	register_ms_ = now_ms() - t0;
	if (p_.verbose)
		std::fprintf(stderr, "[goicp] register %.2f ms: inner BnB rounds %.2f ms (%lld launches: host build %.2f, GPU wait %.2f, host digest %.2f), ICP + DT re-score %.2f ms (%lld passes)\n",
		             register_ms_, bnb_ms_, cnt_.bounds_launches, t_submit_, t_wait_, t_collect_, icp_ms_, cnt_.icp_iters);
	if (p_.verbose) {
		std::fprintf(stderr, "[goicp] translation expansions by parent depth:");
		for (int l = 0; l < 32; l++) if (level_hist_[l]) std::fprintf(stderr, " %d:%lld", l, level_hist_[l]);
		std::fprintf(stderr, "\n");
		std::fprintf(stderr, "[goicp] device-queue expansions by [selection size][spread of the selection in voxels <=5 <=10 <=20 >20], tile rounds %lld, from tiles %lld:\n", tile_rounds_, cnt_.tile_expansions);
		const char* rows[4] = {"  n < 16 ", " 16..31  ", " 32..63  ", " 64..128 "};
		for (int a = 0; a < 4; a++) std::fprintf(stderr, "[goicp]  %s %12lld %12lld %12lld %12lld\n", rows[a], sel_hist_[a][0], sel_hist_[a][1], sel_hist_[a][2], sel_hist_[a][3]);
	}
	register_end();
}

}  // namespace goicp
