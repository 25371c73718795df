// Host-side construction of the implicit left-balanced k-d tree the NN kernels walk, plus Rodrigues.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <thread>
#include <functional>
#include <mutex>
#include <vector>
#include <atomic>

#include "engine.hpp"

namespace goicp {

// run fn(0..ntasks-1) on up to `threads` host threads (1 = inline); tasks are claimed from a counter
void parallel_tasks(int threads, int ntasks, const std::function<void(int)>& fn)
{
	threads = std::min({threads, ntasks, (int)std::max(1u, std::thread::hardware_concurrency())});
	if (threads <= 1) { for (int t = 0; t < ntasks; t++) fn(t); return; }
	std::atomic<int> next{0};
	std::exception_ptr err;
	std::mutex err_mtx;
	auto worker = [&] {
		try {
			for (int t = next.fetch_add(1); t < ntasks; t = next.fetch_add(1)) fn(t);
		} catch (...) {
			std::lock_guard<std::mutex> lk(err_mtx);
			if (!err) err = std::current_exception();
		}
	};
	std::vector<std::thread> pool;
	for (int i = 1; i < threads; i++) pool.emplace_back(worker);
	worker();
	for (auto& th : pool) th.join();
	if (err) std::rethrow_exception(err);
}

// Balanced binary k-d tree by median splits along the widest extent, of the smallest depth D whose
// 2^D leaves hold <= leaf_max points each, flattened into K = ceil(D/6) levels of 64-ary box groups.
// The ROOT group is the sparse one: it has F = 2^(D - 6(K-1)) real children (the binary nodes at that
// depth; the other child slots are empty boxes at distance +inf, which a walk enters only while its
// bound is not yet a finite distance -- the k-NN walk while its list is short.  Never here: the real
// children are taken first and hold all M >= k points.  The device build's empty leaves are entered
// that way, kdbuild.hip), every group below has 64.  A level-l group (l >= 1) is the binary node at depth d_l = log2(F) + 6(l-1) with index g, its
// children are the nodes 6 binary levels below (g*64 + c): the walker's node arithmetic needs no
// child pointers and no per-level fan-out.  Sizing the depth to the cloud keeps leaves full (100 k
// points: 8 192 leaves of 12 instead of 262 144 leaves of 0.4; 1 M: 65 536 of 15 instead of 262 144 of 4).
void build_kdtree(const float* xyz, int M, int leaf_max, KdHost* out)
{
	int D = 0;
	while (D < 6 * kMaxLevels && ((long long)leaf_max << D) < (long long)M) D++;
	if (((long long)leaf_max << D) < (long long)M) throw std::invalid_argument("goicp: target cloud too large for the k-d tree");
	const int K = std::max(1, (D + 5) / 6), L = 1 << D;
	const int d1 = D - 6 * (K - 1);              // binary depth of the root group's children; F = 2^d1
	out->K = K; out->L = L;
	std::vector<int> idx(M);
	std::iota(idx.begin(), idx.end(), 0);
	std::vector<int> lo(2 * (size_t)L, 0), hi(2 * (size_t)L, 0);   // heap order: node n -> children 2n, 2n+1
	lo[1] = 0; hi[1] = M;
	auto split_node = [&](int n) {
		const int a = lo[n], b = hi[n];
		const int mid = a + (b - a) / 2;
		if (b - a > 1) {
			float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
			for (int i = a; i < b; i++)
				for (int k = 0; k < 3; k++) {
					float v = xyz[3 * idx[i] + k];
					mn[k] = std::min(mn[k], v);
					mx[k] = std::max(mx[k], v);
				}
			int dim = 0;
			if (mx[1] - mn[1] > mx[dim] - mn[dim]) dim = 1;
			if (mx[2] - mn[2] > mx[dim] - mn[dim]) dim = 2;
			std::nth_element(idx.begin() + a, idx.begin() + mid, idx.begin() + b, [&](int p, int q) {
				float fp = xyz[3 * p + dim], fq = xyz[3 * q + dim];
				return fp < fq || (fp == fq && p < q);
			});
		}
		lo[2 * (size_t)n] = a; hi[2 * (size_t)n] = mid;
		lo[2 * (size_t)n + 1] = mid; hi[2 * (size_t)n + 1] = b;
	};
	// the four top levels level by level (1, 2, 4, 8 nodes side by side), then the 16 subtrees below them in parallel (disjoint
	// index ranges and heap slots; the result does not depend on the schedule): 1 M points in ~0.1 s
	// instead of 0.35 s
	constexpr int kTop = 16;
	const int threads = M >= (1 << 13) ? kTop : 1;
	for (int d = 0; (1 << d) < std::min(kTop, L); d++)
		parallel_tasks(threads, 1 << d, [&](int t) { split_node((1 << d) + t); });
	if (L > kTop)
		parallel_tasks(threads, kTop, [&](int t) {
			for (int d = 0; ((kTop + t) << d) < L; d++)
				for (int n = (kTop + t) << d; n < ((kTop + t + 1) << d); n++) split_node(n);
		});
	// leaves: node L + f, left to right
	float pad_w;
	const int pad_id = INT32_MAX;
	std::memcpy(&pad_w, &pad_id, sizeof(float));
	out->pts.assign((size_t)L * kLeafSlots, make_float4(INFINITY, INFINITY, INFINITY, pad_w));
	struct Box { float lo[3], hi[3]; };
	std::vector<Box> box(2 * (size_t)L);
	for (auto& bx : box) for (int k = 0; k < 3; k++) { bx.lo[k] = INFINITY; bx.hi[k] = -INFINITY; }
	for (int f = 0; f < L; f++) {
		const int a = lo[(size_t)L + f], b = hi[(size_t)L + f];
		for (int i = a; i < b; i++) {
			const int id = idx[i];
			float w;
			std::memcpy(&w, &id, sizeof(float));
			out->pts[(size_t)f * kLeafSlots + (i - a)] = make_float4(xyz[3 * id], xyz[3 * id + 1], xyz[3 * id + 2], w);
			for (int k = 0; k < 3; k++) {
				box[(size_t)L + f].lo[k] = std::min(box[(size_t)L + f].lo[k], xyz[3 * id + k]);
				box[(size_t)L + f].hi[k] = std::max(box[(size_t)L + f].hi[k], xyz[3 * id + k]);
			}
		}
	}
	for (int n = L - 1; n >= 1; n--)
		for (int k = 0; k < 3; k++) {
			box[n].lo[k] = std::min(box[2 * (size_t)n].lo[k], box[2 * (size_t)n + 1].lo[k]);
			box[n].hi[k] = std::max(box[2 * (size_t)n].hi[k], box[2 * (size_t)n + 1].hi[k]);
		}
	// level 0: the root group, children = the F nodes at depth d1; level l >= 1: the 2^(d1 + 6(l-1))
	// nodes at that depth, children = the nodes 6 levels below
	const Box empty{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
	out->boxes.assign(K, std::vector<float>());
	for (int l = 0; l < K; l++) {
		const int dg = l == 0 ? 0 : d1 + 6 * (l - 1), dc = l == 0 ? d1 : dg + 6;   // depth of the groups / of their children
		const size_t groups = (size_t)1 << dg, fan = (size_t)1 << (dc - dg);
		out->boxes[l].assign(groups * 384, 0.f);
		for (size_t g = 0; g < groups; g++)
			for (size_t c = 0; c < 64; c++) {
				const Box& bx = c < fan ? box[((size_t)1 << dc) + g * fan + c] : empty;
				float* rec = &out->boxes[l][g * 384];
				for (int k = 0; k < 3; k++) { rec[64 * k + c] = bx.lo[k]; rec[192 + 64 * k + c] = bx.hi[k]; }
			}
	}
}

void rodrigues(float ax, float ay, float az, float R[9])
{
	// angle-axis vector (a rotation-cube centre) -> rotation matrix.  Float arithmetic with the same
	// operation order as GoICP::OuterBnB (jly_goicp.cpp:449-467), so R is bit-identical to the CPU path's.
	const float theta = std::sqrt(ax * ax + ay * ay + az * az);
	if (!(theta > 0.f)) {
		for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f;
		return;
	}
	const float ux = ax / theta, uy = ay / theta, uz = az / theta;   // unit axis
	const float c = std::cos(theta), omc = 1 - c, sn = std::sin(theta);
	const float xy = ux * uy * omc, xz = ux * uz * omc, yz = uy * uz * omc;
	const float zs = uz * sn, ys = uy * sn, xs = ux * sn;
	R[0] = c + ux * ux * omc; R[1] = xy - zs;           R[2] = xz + ys;
	R[3] = xy + zs;           R[4] = c + uy * uy * omc; R[5] = yz - xs;
	R[6] = xz - ys;           R[7] = yz + xs;           R[8] = c + uz * uz * omc;
}

namespace {

uint32_t part1by2(uint32_t x)
{
	x &= 0x3ff;
	x = (x ^ (x << 16)) & 0xff0000ff;
	x = (x ^ (x << 8)) & 0x0300f00f;
	x = (x ^ (x << 4)) & 0x030c30c3;
	x = (x ^ (x << 2)) & 0x09249249;
	return x;
}

}  // namespace

void source_morton_frame(const float* source, size_t N, float mn[3], float* ext)
{
	float mx[3] = {-INFINITY, -INFINITY, -INFINITY};
	mn[0] = mn[1] = mn[2] = INFINITY;
	for (size_t i = 0; i < N; i++)
		for (int k = 0; k < 3; k++) {
			mn[k] = std::min(mn[k], source[3 * i + k]);
			mx[k] = std::max(mx[k], source[3 * i + k]);
		}
	*ext = std::max({mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2], 1e-30f});
}

// The source order of Params::morton_sort (0 input order, 1 Morton curve, 2 k-d order): perm[sorted position] = original index
void source_order_host(const float* source, size_t N_, int mode, int32_t* perm_out)
{
	std::vector<int32_t> perm(N_);
	for (size_t i = 0; i < N_; i++) perm[i] = (int32_t)i;
	if (mode == 1) {
		float mn[3], ext;
		source_morton_frame(source, N_, mn, &ext);
		std::vector<uint32_t> code(N_);
		for (size_t i = 0; i < N_; i++) {
			uint32_t c = 0;
			for (int k = 0; k < 3; k++) {
				float f = (source[3 * i + k] - mn[k]) / ext;
				uint32_t q = (uint32_t)std::min(1023.f, std::max(0.f, f * 1024.f));
				c |= part1by2(q) << k;
			}
			code[i] = c;
		}
		std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return code[a] < code[b]; });
	} else if (mode >= 2) {
		// k-d order: split the longest axis of the subset's bounding box at the median, rounded so that
		// the left part holds a multiple of 256 / 64 / 16 / 4 points (the largest that is smaller than the
		// subset), down to single points.  Every aligned run of 64 points (one wavefront's gathers) is
		// then a compact box-shaped surface patch, every aligned 4 and 16 lanes a sub-patch of it, and
		// every aligned 256 (one workgroup iteration) a subtree: fewer distinct DT cache lines per gather
		// instruction than a space-filling curve gives.  65 536-cube launch on the bunny: Morton 2.28 ms,
		// Hilbert 2.13 ms, 64-point clusters 1.94 ms (principal-axis splits 2.01 ms), clusters ordered
		// down to 4 points 1.85 ms, down to single points 1.84 ms.
		// The result is unique whatever nth_element does inside a half: the size of the left part depends on the
		// run's length only (source_order_left), the comparator is a total order, and the recursion ends at single
		// points -- which is what lets the device build the same permutation level by level (kdbuild.hip)
		// one split; returns the size of the left part (0 = nothing to split)
		auto split = [&](size_t lo, size_t hi) -> size_t {
			const size_t n = hi - lo;
			if (n <= 1) return 0;
			float bmn[3] = {INFINITY, INFINITY, INFINITY}, bmx[3] = {-INFINITY, -INFINITY, -INFINITY};
			for (size_t i = lo; i < hi; i++)
				for (int k = 0; k < 3; k++) {
					bmn[k] = std::min(bmn[k], source[3 * perm[i] + k]);
					bmx[k] = std::max(bmx[k], source[3 * perm[i] + k]);
				}
			int ax = 0;
			for (int k = 1; k < 3; k++) if (bmx[k] - bmn[k] > bmx[ax] - bmn[ax]) ax = k;
			const size_t nl = (size_t)source_order_left((int)n);
			std::nth_element(perm.begin() + lo, perm.begin() + lo + nl, perm.begin() + hi, [&](int32_t a, int32_t b) {
				const float fa = source[3 * a + ax], fb = source[3 * b + ax];
				return fa < fb || (fa == fb && a < b);                    // total order: the permutation is reproducible
			});
			return nl;
		};
		auto order_range = [&](size_t lo0, size_t hi0) {
			std::vector<std::pair<size_t, size_t>> stack{{lo0, hi0}};
			while (!stack.empty()) {
				auto [lo, hi] = stack.back(); stack.pop_back();
				const size_t nl = split(lo, hi);
				if (!nl) continue;
				stack.push_back({lo + nl, hi});
				stack.push_back({lo, lo + nl});
			}
		};
		// the top of the tree level by level (its 1, 2, 4, 8 splits side by side), the (<= 16) ranges below in parallel
		std::vector<std::pair<size_t, size_t>> ranges{{0, N_}};
		while (N_ >= (1u << 13) && ranges.size() < 16) {
			std::vector<size_t> nls(ranges.size());
			parallel_tasks(16, (int)ranges.size(), [&](int t) { nls[t] = split(ranges[t].first, ranges[t].second); });
			std::vector<std::pair<size_t, size_t>> next;
			for (size_t t = 0; t < ranges.size(); t++) {
				const auto [lo, hi] = ranges[t];
				if (nls[t]) { next.push_back({lo, lo + nls[t]}); next.push_back({lo + nls[t], hi}); } else next.push_back({lo, hi});
			}
			if (next.size() == ranges.size()) break;
			ranges.swap(next);
		}
		parallel_tasks(16, (int)ranges.size(), [&](int t) { order_range(ranges[t].first, ranges[t].second); });
	}
	std::memcpy(perm_out, perm.data(), sizeof(int32_t) * N_);
}

// ---- voxel-grid downsampling: the frame both paths share, and the host path ----
// what follows the scan of the cloud: the limits on E and the derived fields.  radius > 0: the radius filter's grid, with its 2^16 rule
static void fill_frame(const float mn[3], float E, size_t n, float voxel, float radius, VoxelFrame* f)
{
	if (radius > 0.f && !(E / radius < 65536.f)) throw std::invalid_argument("goicp outlier: the grid needs more than 16 bits per axis (extent / radius >= 2^16)");
	if (!(E / voxel < 2097152.f)) throw std::invalid_argument("goicp voxel: the grid needs more than 21 bits per axis (extent / voxel >= 2^21)");
	for (int k = 0; k < 3; k++) f->mn[k] = mn[k];
	f->E = E;
	f->voxel = voxel;
	f->s = 0;
	if (E > 0.f) {
		int e = 0, b = 0;
		std::frexp(E, &e);                             // E < 2^e
		for (size_t v = n; v; v >>= 1) b++;            // n < 2^b
		f->s = 62 - e - b;                             // every term < 2^(62-b), fewer than 2^b of them: the sums stay below 2^62
	}
	int cbits = 0;
	for (int c = (int)std::floor(E / voxel); c; c >>= 1) cbits++;
	f->key_bits = 42 + std::max(cbits, 1);
}

// radius > 0: the frame of the radius filter's grid (pitch `voxel` = radius * 1.03125f), which adds the 2^16 rule
static void grid_frame(const float* xyz, size_t n, float voxel, float radius, VoxelFrame* f)
{
	if (!xyz || n == 0) throw std::invalid_argument("goicp voxel: empty cloud");
	if (n > (size_t)INT32_MAX / 8) throw std::invalid_argument("goicp voxel: cloud too large");
	if (!(voxel > 0.f) || !std::isfinite(voxel)) throw std::invalid_argument("goicp voxel: the voxel size must be positive and finite");
	float mn[3] = {INFINITY, INFINITY, INFINITY};
	for (size_t i = 0; i < n; i++)
		for (int k = 0; k < 3; k++) {
			const float x = xyz[3 * i + k];
			if (!std::isfinite(x)) throw std::invalid_argument("goicp voxel: non-finite coordinate in the cloud");
			mn[k] = std::min(mn[k], x);
		}
	float E = 0.f;
	for (size_t i = 0; i < n; i++)
		for (int k = 0; k < 3; k++) E = std::max(E, xyz[3 * i + k] - mn[k]);
	fill_frame(mn, E, n, voxel, radius, f);
}

void voxel_frame(const float* xyz, size_t n, float voxel, VoxelFrame* f) { grid_frame(xyz, n, voxel, 0.f, f); }

void radius_check_params(float radius, int32_t min_neighbors)
{
	if (!(radius > 0.f) || !std::isfinite(radius)) throw std::invalid_argument("goicp outlier: the radius must be positive and finite");
	if (!std::isnormal(radius * radius)) throw std::invalid_argument("goicp outlier: radius * radius must be a normal float");
	if (min_neighbors < 1) throw std::invalid_argument("goicp outlier: min_neighbors must be at least 1");
}

void radius_frame(const float* xyz, size_t n, float radius, int32_t min_neighbors, VoxelFrame* f)
{
	if (!xyz || n == 0) throw std::invalid_argument("goicp outlier: empty cloud");
	if (n > (size_t)INT32_MAX / 8) throw std::invalid_argument("goicp outlier: cloud too large");
	radius_check_params(radius, min_neighbors);
	grid_frame(xyz, n, radius * 1.03125f, radius, f);
}

void radius_frame_of_box(const float mn[3], const float mx[3], size_t n, float radius, int32_t min_neighbors, VoxelFrame* f)
{
	radius_check_params(radius, min_neighbors);
	float E = 0.f;
	for (int k = 0; k < 3; k++) E = std::max(E, mx[k] - mn[k]);   // rounding is monotone: the largest offset is the one of an axis' maximum
	fill_frame(mn, E, n, radius * 1.03125f, radius, f);
}

void voxel_downsample_host(const float* xyz, size_t n, float voxel, float* out_xyz, int32_t* out_count, size_t* m_out)
{
	VoxelFrame f;
	voxel_frame(xyz, n, voxel, &f);
	std::vector<std::pair<uint64_t, int32_t>> ki(n);
	for (size_t i = 0; i < n; i++) {
		uint64_t key = 0;
		for (int k = 0; k < 3; k++) key |= (uint64_t)(int)std::floor((xyz[3 * i + k] - f.mn[k]) / voxel) << (21 * k);
		ki[i] = {key, (int32_t)i};
	}
	std::sort(ki.begin(), ki.end());                   // (key, id): the ids of a cell ascend, as after a stable sort
	size_t m = 0;
	for (size_t a = 0; a < n;) {
		size_t b = a;
		long long S[3] = {0, 0, 0};
		for (; b < n && ki[b].first == ki[a].first; b++) {
			const float* p = xyz + 3 * (size_t)ki[b].second;
			for (int k = 0; k < 3; k++) S[k] += std::llrint(std::ldexp((double)(p[k] - f.mn[k]), f.s));
		}
		const size_t cnt = b - a;
		const float* p = xyz + 3 * (size_t)ki[a].second;
		for (int k = 0; k < 3; k++)
			out_xyz[3 * m + k] = cnt == 1 ? p[k] : (float)((double)f.mn[k] + std::ldexp((double)S[k] / (double)cnt, -f.s));
		if (out_count) out_count[m] = (int32_t)cnt;
		m++;
		a = b;
	}
	*m_out = m;
}

// ---- radius outlier removal: the host path.  The points are sorted by the key of their cell (pitch 1.03125 r); the 27 cells
// around a point are 9 runs of up to three consecutive keys, each one lower and one upper binary search; a point leaves its loop once it
// has min_neighbors.  The grid only selects candidates: what counts is the float expression of the header ----
void radius_outlier_removal_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, float* out_xyz, int32_t* out_index,
                                 int32_t* out_count, size_t* m_out)
{
	VoxelFrame f;
	radius_frame(xyz, n, radius, min_neighbors, &f);
	const float r2 = radius * radius;
	std::vector<std::pair<uint64_t, int32_t>> ki(n);
	for (size_t i = 0; i < n; i++) {
		uint64_t key = 0;
		for (int k = 0; k < 3; k++) key |= (uint64_t)(int)std::floor((xyz[3 * i + k] - f.mn[k]) / f.voxel) << (21 * k);
		ki[i] = {key, (int32_t)i};
	}
	std::sort(ki.begin(), ki.end());
	struct Pt { float x, y, z; int32_t id; };
	std::vector<uint64_t> keys(n);
	std::vector<Pt> pts(n);
	for (size_t s = 0; s < n; s++) {
		const float* p = xyz + 3 * (size_t)ki[s].second;
		keys[s] = ki[s].first;
		pts[s] = {p[0], p[1], p[2], ki[s].second};
	}
	std::vector<std::pair<uint64_t, int32_t>>().swap(ki);
	std::vector<int32_t> count(n);
	const size_t chunk = 4096, chunks = (n + chunk - 1) / chunk;
	parallel_tasks(n >= 65536 ? 8 : 1, (int)chunks, [&](int t) {
		for (size_t s = (size_t)t * chunk; s < std::min(n, ((size_t)t + 1) * chunk); s++) {
			const Pt P = pts[s];
			const int64_t cx = (int64_t)(keys[s] & 0x1fffffu), cy = (int64_t)((keys[s] >> 21) & 0x1fffffu), cz = (int64_t)(keys[s] >> 42);
			int32_t cnt = 0;
			for (int64_t z = std::max<int64_t>(cz - 1, 0); z <= cz + 1 && cnt < min_neighbors; z++)       // clamped at the low faces; past the
				for (int64_t y = std::max<int64_t>(cy - 1, 0); y <= cy + 1 && cnt < min_neighbors; y++) {   // high ones there are no keys
					const uint64_t base = ((uint64_t)z << 42) | ((uint64_t)y << 21);
					const size_t a = std::lower_bound(keys.begin(), keys.end(), base | (uint64_t)std::max<int64_t>(cx - 1, 0)) - keys.begin();
					const size_t b = std::upper_bound(keys.begin() + a, keys.end(), base | (uint64_t)(cx + 1)) - keys.begin();
					for (size_t j = a; j < b && cnt < min_neighbors; j++) {
						const Pt& Q = pts[j];
						if (Q.id == P.id) continue;
						const float dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
						const float d2 = dx * dx + dy * dy + dz * dz;
						if (d2 <= r2) cnt++;
					}
				}
			count[(size_t)P.id] = cnt;
		}
	});
	size_t m = 0;
	for (size_t i = 0; i < n; i++) {
		if (out_count) out_count[i] = count[i];
		if (count[i] != min_neighbors) continue;
		for (int k = 0; k < 3; k++) out_xyz[3 * m + k] = xyz[3 * i + k];
		if (out_index) out_index[m] = (int32_t)i;
		m++;
	}
	*m_out = m;
}

// ---- Euclidean / DBSCAN clustering: what both paths share, and the host path ----
// the radius filter's frame and refusals, except that min_neighbors == 0 (every point is core) is legal
void cluster_frame(const float* xyz, size_t n, float radius, int32_t min_neighbors, VoxelFrame* f)
{
	if (min_neighbors < 0) throw std::invalid_argument("goicp cluster: min_neighbors must not be negative");
	radius_frame(xyz, n, radius, std::max(min_neighbors, 1), f);
}

void cluster_frame_of_box(const float mn[3], const float mx[3], size_t n, float radius, int32_t min_neighbors, VoxelFrame* f)
{
	if (min_neighbors < 0) throw std::invalid_argument("goicp cluster: min_neighbors must not be negative");
	radius_frame_of_box(mn, mx, n, radius, std::max(min_neighbors, 1), f);
}

void cluster_check_select(int32_t min_size, int32_t max_clusters)
{
	if (min_size < 0) throw std::invalid_argument("goicp cluster: min_size must not be negative");
	if (max_clusters < 0) throw std::invalid_argument("goicp cluster: max_clusters must not be negative");
}

// keep[l] = 1 for the clusters the selection keeps: ranked by size descending, ties to the smaller label, the first max_clusters (0 = all) of
// those with size >= max(min_size, 1)
void cluster_select(const int32_t* sizes, size_t c, int32_t min_size, int32_t max_clusters, std::vector<int32_t>* keep)
{
	keep->assign(c, 0);
	std::vector<uint64_t> rank(c);
	for (size_t l = 0; l < c; l++) rank[l] = ((uint64_t)(uint32_t)(INT32_MAX - sizes[l]) << 32) | (uint64_t)l;
	std::sort(rank.begin(), rank.end());
	const size_t limit = max_clusters > 0 ? std::min<size_t>((size_t)max_clusters, c) : c;
	for (size_t k = 0; k < limit; k++) {
		const size_t l = (size_t)(rank[k] & 0xffffffffu);
		if (sizes[l] >= std::max(min_size, 1)) (*keep)[l] = 1;
	}
}

// The radius filter's sorted cells and 27-cell candidate runs.  Pass 1 is its saturating count (the core flag), pass 2 a sequential
// union-find over the core pairs (the larger root goes under the smaller, so a component's root is its smallest core index), pass 3 the
// border points' smallest key over their core neighbours, then the relabelling in ascending root order
void cluster_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t* out_label, int32_t* out_sizes, size_t* c_out)
{
	VoxelFrame f;
	cluster_frame(xyz, n, radius, min_neighbors, &f);
	const float r2 = radius * radius;
	std::vector<std::pair<uint64_t, int32_t>> ki(n);
	for (size_t i = 0; i < n; i++) {
		uint64_t key = 0;
		for (int k = 0; k < 3; k++) key |= (uint64_t)(int)std::floor((xyz[3 * i + k] - f.mn[k]) / f.voxel) << (21 * k);
		ki[i] = {key, (int32_t)i};
	}
	std::sort(ki.begin(), ki.end());
	struct Pt { float x, y, z; int32_t id; };
	std::vector<uint64_t> keys(n);
	std::vector<Pt> pts(n);
	for (size_t s = 0; s < n; s++) {
		const float* p = xyz + 3 * (size_t)ki[s].second;
		keys[s] = ki[s].first;
		pts[s] = {p[0], p[1], p[2], ki[s].second};
	}
	std::vector<std::pair<uint64_t, int32_t>>().swap(ki);
	// fn(Q, d2) for every other point Q of the 27 cells around sorted position s that lies within r; fn returns false to stop
	auto neighbours = [&](size_t s, auto&& fn) {
		const Pt P = pts[s];
		const int64_t cx = (int64_t)(keys[s] & 0x1fffffu), cy = (int64_t)((keys[s] >> 21) & 0x1fffffu), cz = (int64_t)(keys[s] >> 42);
		for (int64_t z = std::max<int64_t>(cz - 1, 0); z <= cz + 1; z++)
			for (int64_t y = std::max<int64_t>(cy - 1, 0); y <= cy + 1; y++) {
				const uint64_t base = ((uint64_t)z << 42) | ((uint64_t)y << 21);
				const size_t a = std::lower_bound(keys.begin(), keys.end(), base | (uint64_t)std::max<int64_t>(cx - 1, 0)) - keys.begin();
				const size_t b = std::upper_bound(keys.begin() + a, keys.end(), base | (uint64_t)(cx + 1)) - keys.begin();
				for (size_t j = a; j < b; j++) {
					const Pt& Q = pts[j];
					if (Q.id == P.id) continue;
					const float dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
					const float d2 = dx * dx + dy * dy + dz * dz;
					if (d2 <= r2 && !fn(Q, d2)) return;
				}
			}
	};
	std::vector<char> core(n, 1);
	if (min_neighbors > 0) {
		const size_t chunk = 4096, chunks = (n + chunk - 1) / chunk;
		parallel_tasks(n >= 65536 ? 8 : 1, (int)chunks, [&](int t) {
			for (size_t s = (size_t)t * chunk; s < std::min(n, ((size_t)t + 1) * chunk); s++) {
				int32_t cnt = 0;
				neighbours(s, [&](const Pt&, float) { return ++cnt < min_neighbors; });
				core[(size_t)pts[s].id] = cnt == min_neighbors;
			}
		});
	}
	std::vector<int32_t> parent(n);
	for (size_t i = 0; i < n; i++) parent[i] = (int32_t)i;
	auto find = [&](int32_t x) {
		while (parent[(size_t)x] != x) {
			parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];   // path halving
			x = parent[(size_t)x];
		}
		return x;
	};
	for (size_t s = 0; s < n; s++) {
		const int32_t i = pts[s].id;
		if (!core[(size_t)i]) continue;
		neighbours(s, [&](const Pt& Q, float) {
			if (Q.id < i && core[(size_t)Q.id]) {
				const int32_t a = find(i), b = find(Q.id);
				if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
			}
			return true;
		});
	}
	// root[i]: the smallest core index of i's cluster, -1 for noise
	std::vector<int32_t> root(n, -1);
	for (size_t i = 0; i < n; i++) if (core[i]) root[i] = find((int32_t)i);
	for (size_t s = 0; s < n; s++) {
		const int32_t i = pts[s].id;
		if (core[(size_t)i]) continue;
		uint64_t best = UINT64_MAX;
		neighbours(s, [&](const Pt& Q, float d2) {
			if (core[(size_t)Q.id]) {
				uint32_t bits;
				std::memcpy(&bits, &d2, sizeof(bits));
				best = std::min(best, ((uint64_t)bits << 32) | (uint64_t)(uint32_t)Q.id);
			}
			return true;
		});
		if (best != UINT64_MAX) root[(size_t)i] = root[(size_t)(best & 0xffffffffu)];
	}
	std::vector<int32_t> dense(n, -1);
	size_t c = 0;
	for (size_t i = 0; i < n; i++) if (root[i] == (int32_t)i) dense[i] = (int32_t)c++;
	if (out_sizes) for (size_t l = 0; l < c; l++) out_sizes[l] = 0;
	for (size_t i = 0; i < n; i++) {
		const int32_t l = root[i] < 0 ? -1 : dense[(size_t)root[i]];
		out_label[i] = l;
		if (out_sizes && l >= 0) out_sizes[(size_t)l]++;
	}
	*c_out = c;
}

void cluster_filter_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t min_size, int32_t max_clusters, float* out_xyz,
                         int32_t* out_index, int32_t* out_label, size_t* m_out)
{
	cluster_check_select(min_size, max_clusters);
	std::vector<int32_t> label(n), sizes(n), keep;
	size_t c = 0;
	cluster_host(xyz, n, radius, min_neighbors, label.data(), sizes.data(), &c);
	cluster_select(sizes.data(), c, min_size, max_clusters, &keep);
	size_t m = 0;
	for (size_t i = 0; i < n; i++) {
		if (label[i] < 0 || !keep[(size_t)label[i]]) continue;
		for (int k = 0; k < 3; k++) out_xyz[3 * m + k] = xyz[3 * i + k];
		if (out_index) out_index[m] = (int32_t)i;
		if (out_label) out_label[m] = label[i];
		m++;
	}
	*m_out = m;
}

// ---- statistical outlier removal: what both paths share, and the host path ----
void stat_check_params(size_t n, int32_t neighbors, float std_ratio)
{
	if (neighbors < 1 || neighbors > 64) throw std::invalid_argument("goicp stat outlier: neighbors must be in 1..64");
	if (n == 0 || (size_t)neighbors > n - 1) throw std::invalid_argument("goicp stat outlier: neighbors must be at most n - 1");
	if (!std::isfinite(std_ratio) || std_ratio < 0.f) throw std::invalid_argument("goicp stat outlier: std_ratio must be finite and >= 0");
}

void stat_check_cloud(const float* xyz, size_t n, float mn[3], float mx[3])
{
	if (!xyz || n == 0) throw std::invalid_argument("goicp stat outlier: empty cloud");
	if (n > (size_t)INT32_MAX / 8) throw std::invalid_argument("goicp stat outlier: cloud too large");
	for (int k = 0; k < 3; k++) { mn[k] = INFINITY; mx[k] = -INFINITY; }
	for (size_t i = 0; i < n; i++)
		for (int k = 0; k < 3; k++) {
			const float x = xyz[3 * i + k];
			if (!std::isfinite(x)) throw std::invalid_argument("goicp stat outlier: non-finite coordinate in the cloud");
			mn[k] = std::min(mn[k], x);
			mx[k] = std::max(mx[k], x);
		}
}

// The first radius only decides how much work the levels do, never a bit of the result, so it is an estimate from a sample: the median
// distance r_s from a sample point to its 8th nearest in the sample (ns points, every (n / ns)-th of the cloud), scaled to the radius that
// holds 2 k points of the whole cloud as if the cloud were locally three-dimensional, r_s cbrt(2 k ns / (8 n)) -- a surface scan then gets
// a few times more candidates than it needs, never fewer.  The median does not move with a few far points, which is what the extent E
// would do; without a usable sample (none given, or r_s == 0) the fallback is E cbrt(k / n), a cloud that fills its bounding cube
static float stat_r0_estimate(const float* sample, size_t ns, size_t n, int32_t neighbors)
{
	if (!sample || ns < 16) return 0.f;
	const size_t m = std::min<size_t>(8, ns - 1), step = std::max<size_t>(1, ns / 256);
	std::vector<float> d2(ns), rs;
	for (size_t i = 0; i < ns; i += step) {
		for (size_t j = 0; j < ns; j++) {
			const float dx = sample[3 * i] - sample[3 * j], dy = sample[3 * i + 1] - sample[3 * j + 1], dz = sample[3 * i + 2] - sample[3 * j + 2];
			d2[j] = dx * dx + dy * dy + dz * dz;
		}
		d2[i] = INFINITY;
		std::nth_element(d2.begin(), d2.begin() + (m - 1), d2.end());
		rs.push_back(std::sqrt(d2[m - 1]));
	}
	std::nth_element(rs.begin(), rs.begin() + rs.size() / 2, rs.end());
	const float r_s = rs[rs.size() / 2];
	if (!(r_s > 0.f) || !std::isfinite(r_s)) return 0.f;
	return r_s * std::cbrt(2.f * (float)neighbors * (float)ns / ((float)m * (float)n));
}

size_t stat_sample_size(size_t n) { return std::min<size_t>(n, 4096); }

// Clamped to [E 2^-15, E]; no grid level (r0 = 0) when E == 0 or r0 * r0 is no normal float.  The level radii double up to the first
// two that reach 2 E (where one cell holds the cloud) or until their square overflows; what is left after them goes to the top level
void stat_levels(const float mn[3], const float mx[3], size_t n, int32_t neighbors, const float* sample, size_t ns, float* r0_out, int* levels_out)
{
	*r0_out = 0.f;
	*levels_out = 0;
	float E = 0.f;
	for (int k = 0; k < 3; k++) E = std::max(E, mx[k] - mn[k]);
	if (!(E > 0.f) || !std::isfinite(E)) return;
	float r0 = stat_r0_estimate(sample, ns, n, neighbors);
	if (!(r0 > 0.f) || !std::isfinite(r0)) r0 = E * std::cbrt((float)neighbors / (float)n);
	r0 = std::min(r0, E);
	if (!(E / r0 < 32768.f)) r0 = E * (1.f / 32768.f);
	if (!std::isnormal(r0 * r0) || !(E / r0 < 65536.f)) return;
	int cap = 2;
	for (float r = r0; r < E && cap < 40; r *= 2.f) cap++;
	int levels = 0;
	for (float r = r0; levels < cap && std::isnormal(r * r) && std::isfinite(r * 1.03125f); r *= 2.f) levels++;
	*r0_out = r0;
	*levels_out = levels;
}

namespace {

// the k smallest d2 of a point, kept as a max-heap of at most k values
struct StatHeap {
	float h[64];
	int size = 0, k;
	explicit StatHeap(int k_) : k(k_) {}
	void offer(float d2)
	{
		if (size < k) { h[size++] = d2; std::push_heap(h, h + size); }
		else if (d2 < h[0]) { std::pop_heap(h, h + k); h[k - 1] = d2; std::push_heap(h, h + k); }
	}
	bool within(float r2) const { return size == k && h[0] <= r2; }
	float mean()
	{
		std::sort(h, h + k);
		double s = 0.0;
		for (int j = 0; j < k; j++) s += (double)std::sqrt(h[j]);
		return (float)(s / (double)k);
	}
};

inline float stat_d2(const float* p, const float* q)
{
	const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
	return dx * dx + dy * dy + dz * dz;
}

}  // namespace

void statistical_outlier_removal_host(const float* xyz, size_t n, int32_t neighbors, float std_ratio, float* out_xyz, int32_t* out_index,
                                      float* out_mean_dist, double* threshold, size_t* m_out)
{
	float mn[3], mx[3];
	stat_check_cloud(xyz, n, mn, mx);
	stat_check_params(n, neighbors, std_ratio);
	const int k = neighbors;
	float r0 = 0.f;
	int levels = 0;
	{
		// every (n / ns)-th point of the cloud
		const size_t ns = stat_sample_size(n), stride = n / ns;
		std::vector<float> sample(3 * ns);
		for (size_t i = 0; i < ns; i++) std::memcpy(&sample[3 * i], xyz + 3 * i * stride, 3 * sizeof(float));
		stat_levels(mn, mx, n, k, sample.data(), ns, &r0, &levels);
	}
	std::vector<float> u(n);
	std::vector<int32_t> list(n), next;
	std::iota(list.begin(), list.end(), 0);
	const int threads = n >= 65536 ? 8 : 1;
	const size_t chunk = 4096;
	struct Pt { float x, y, z; int32_t id; };
	std::vector<uint64_t> keys;
	std::vector<Pt> pts;
	std::vector<std::pair<uint64_t, int32_t>> ki;
	std::vector<unsigned char> open;
	float r = r0;
	for (int L = 0; L < levels && !list.empty(); L++, r *= 2.f) {
		VoxelFrame f;
		radius_frame_of_box(mn, mx, n, r, 1, &f);
		const float r2 = r * r;
		auto key_of = [&](const float* p) {
			uint64_t key = 0;
			for (int a = 0; a < 3; a++) key |= (uint64_t)(int)std::floor((p[a] - f.mn[a]) / f.voxel) << (21 * a);
			return key;
		};
		ki.resize(n);
		for (size_t i = 0; i < n; i++) ki[i] = {key_of(xyz + 3 * i), (int32_t)i};
		std::sort(ki.begin(), ki.end());
		keys.resize(n); pts.resize(n);
		for (size_t s = 0; s < n; s++) {
			const float* p = xyz + 3 * (size_t)ki[s].second;
			keys[s] = ki[s].first;
			pts[s] = {p[0], p[1], p[2], ki[s].second};
		}
		open.assign(list.size(), 0);
		parallel_tasks(threads, (int)((list.size() + chunk - 1) / chunk), [&](int t) {
			for (size_t e = (size_t)t * chunk; e < std::min(list.size(), ((size_t)t + 1) * chunk); e++) {
				const int32_t id = list[e];
				const float* P = xyz + 3 * (size_t)id;
				const uint64_t K = key_of(P);
				const int64_t cx = (int64_t)(K & 0x1fffffu), cy = (int64_t)((K >> 21) & 0x1fffffu), cz = (int64_t)(K >> 42);
				StatHeap H(k);
				for (int64_t z = std::max<int64_t>(cz - 1, 0); z <= cz + 1; z++)
					for (int64_t y = std::max<int64_t>(cy - 1, 0); y <= cy + 1; y++) {
						const uint64_t base = ((uint64_t)z << 42) | ((uint64_t)y << 21);
						const size_t a = std::lower_bound(keys.begin(), keys.end(), base | (uint64_t)std::max<int64_t>(cx - 1, 0)) - keys.begin();
						const size_t b = std::upper_bound(keys.begin() + a, keys.end(), base | (uint64_t)(cx + 1)) - keys.begin();
						for (size_t j = a; j < b; j++)
							if (pts[j].id != id) H.offer(stat_d2(P, &pts[j].x));
					}
				if (H.within(r2)) u[(size_t)id] = H.mean(); else open[e] = 1;
			}
		});
		next.clear();
		for (size_t e = 0; e < list.size(); e++) if (open[e]) next.push_back(list[e]);
		list.swap(next);
	}
	// the top level: every point is a candidate
	if (!list.empty())
		parallel_tasks(threads, (int)((list.size() + 255) / 256), [&](int t) {
			for (size_t e = (size_t)t * 256; e < std::min(list.size(), ((size_t)t + 1) * 256); e++) {
				const int32_t id = list[e];
				const float* P = xyz + 3 * (size_t)id;
				StatHeap H(k);
				for (size_t j = 0; j < n; j++)
					if ((int32_t)j != id) H.offer(stat_d2(P, xyz + 3 * j));
				u[(size_t)id] = H.mean();
			}
		});
	// the fixed-point image and the finish
	float U = 0.f;
	for (size_t i = 0; i < n; i++) U = std::max(U, u[i]);
	int e = 0;
	double Tq = 0.0, thr = 0.0;
	if (U > 0.f) {
		std::frexp(U, &e);
		int64_t S1 = 0, A = 0, B = 0;
		for (size_t i = 0; i < n; i++) {
			const uint64_t q = (uint64_t)(int64_t)std::floor(std::ldexp((double)u[i], 31 - e));
			S1 += (int64_t)q;
			A += (int64_t)((q * q) >> 32);
			B += (int64_t)((q * q) & 0xffffffffull);
		}
		const double nd = (double)n;
		const double mean = (double)S1 / nd;
		const double S2 = std::ldexp((double)A, 32) + (double)B;
		const double prod = (double)S1 * mean;
		double var = (S2 - prod) / (nd - 1.0);
		if (!(var > 0.0)) var = 0.0;
		const double dev = (double)std_ratio * std::sqrt(var);
		Tq = mean + dev;
		thr = std::ldexp(Tq, e - 31);
	}
	size_t m = 0;
	for (size_t i = 0; i < n; i++) {
		if (out_mean_dist) out_mean_dist[i] = u[i];
		if (U > 0.f && !((double)(int64_t)std::floor(std::ldexp((double)u[i], 31 - e)) <= Tq)) continue;
		for (int a = 0; a < 3; a++) out_xyz[3 * m + a] = xyz[3 * i + a];
		if (out_index) out_index[m] = (int32_t)i;
		m++;
	}
	if (threshold) *threshold = thr;
	*m_out = m;
}

// ---- exact self k-NN and normal estimation: what both paths share, and the host path ----
void knn_self_check_params(size_t n, int32_t k)
{
	if (k < 1 || k > kKnnSelfMax) throw std::invalid_argument("goicp knn self: k must be in 1..32");
	if (n == 0 || (size_t)k > n - 1) throw std::invalid_argument("goicp knn self: k must be at most n - 1");
}

void normals_check_params(size_t n, int32_t k, const float* vp)
{
	if (k < 3 || k > kKnnSelfMax) throw std::invalid_argument("goicp estimate normals: k must be in 3..32 (it counts the point itself)");
	if (n == 0 || (size_t)(k - 1) > n - 1) throw std::invalid_argument("goicp estimate normals: k - 1 must be at most n - 1");
	if (vp && !(std::isfinite(vp[0]) && std::isfinite(vp[1]) && std::isfinite(vp[2]))) throw std::invalid_argument("goicp estimate normals: non-finite viewpoint");
}

namespace {

// the k smallest keys (bits of d2) << 32 | index of a point, kept as a max-heap of at most k keys
struct KeyHeap {
	uint64_t h[kKnnSelfMax];
	int size = 0, k;
	explicit KeyHeap(int k_) : k(k_) {}
	void offer(float d2, int32_t j)
	{
		uint32_t bits;
		std::memcpy(&bits, &d2, sizeof bits);
		const uint64_t key = ((uint64_t)bits << 32) | (uint32_t)j;
		if (size < k) { h[size++] = key; std::push_heap(h, h + size); }
		else if (key < h[0]) { std::pop_heap(h, h + k); h[k - 1] = key; std::push_heap(h, h + k); }
	}
	static float d2_of(uint64_t key)
	{
		const uint32_t bits = (uint32_t)(key >> 32);
		float d2;
		std::memcpy(&d2, &bits, sizeof d2);
		return d2;
	}
	bool within(float r2) const { return size == k && d2_of(h[0]) <= r2; }
	// ascending by key; index (k ints) and dist_sq (k floats, may be null) are the point's own words
	void write(int32_t* index, float* dist_sq)
	{
		std::sort(h, h + k);
		for (int j = 0; j < k; j++) {
			index[j] = (int32_t)(uint32_t)(h[j] & 0xffffffffull);
			if (dist_sq) dist_sq[j] = d2_of(h[j]);
		}
	}
};

// the rows of every point: the level loop of statistical_outlier_removal_host with keys in the heap.  A point is resolved at level L when
// it holds k keys and the d2 of its k-th key is <= r2_L (DESIGN 20 has the proof that the ties at the k-th place are then decided)
void knn_self_rows(const float* xyz, size_t n, int k, const float mn[3], const float mx[3], int32_t* out_index, float* out_dist_sq)
{
	float r0 = 0.f;
	int levels = 0;
	{
		const size_t ns = stat_sample_size(n), stride = n / ns;
		std::vector<float> sample(3 * ns);
		for (size_t i = 0; i < ns; i++) std::memcpy(&sample[3 * i], xyz + 3 * i * stride, 3 * sizeof(float));
		stat_levels(mn, mx, n, k, sample.data(), ns, &r0, &levels);
	}
	std::vector<int32_t> list(n), next;
	std::iota(list.begin(), list.end(), 0);
	const int threads = n >= 65536 ? 8 : 1;
	const size_t chunk = 4096;
	struct Pt { float x, y, z; int32_t id; };
	std::vector<uint64_t> keys;
	std::vector<Pt> pts;
	std::vector<std::pair<uint64_t, int32_t>> ki;
	std::vector<unsigned char> open;
	float r = r0;
	for (int L = 0; L < levels && !list.empty(); L++, r *= 2.f) {
		VoxelFrame f;
		radius_frame_of_box(mn, mx, n, r, 1, &f);
		const float r2 = r * r;
		auto key_of = [&](const float* p) {
			uint64_t key = 0;
			for (int a = 0; a < 3; a++) key |= (uint64_t)(int)std::floor((p[a] - f.mn[a]) / f.voxel) << (21 * a);
			return key;
		};
		ki.resize(n);
		for (size_t i = 0; i < n; i++) ki[i] = {key_of(xyz + 3 * i), (int32_t)i};
		std::sort(ki.begin(), ki.end());
		keys.resize(n); pts.resize(n);
		for (size_t s = 0; s < n; s++) {
			const float* p = xyz + 3 * (size_t)ki[s].second;
			keys[s] = ki[s].first;
			pts[s] = {p[0], p[1], p[2], ki[s].second};
		}
		open.assign(list.size(), 0);
		parallel_tasks(threads, (int)((list.size() + chunk - 1) / chunk), [&](int t) {
			for (size_t e = (size_t)t * chunk; e < std::min(list.size(), ((size_t)t + 1) * chunk); e++) {
				const int32_t id = list[e];
				const float* P = xyz + 3 * (size_t)id;
				const uint64_t K = key_of(P);
				const int64_t cx = (int64_t)(K & 0x1fffffu), cy = (int64_t)((K >> 21) & 0x1fffffu), cz = (int64_t)(K >> 42);
				KeyHeap H(k);
				for (int64_t z = std::max<int64_t>(cz - 1, 0); z <= cz + 1; z++)
					for (int64_t y = std::max<int64_t>(cy - 1, 0); y <= cy + 1; y++) {
						const uint64_t base = ((uint64_t)z << 42) | ((uint64_t)y << 21);
						const size_t a = std::lower_bound(keys.begin(), keys.end(), base | (uint64_t)std::max<int64_t>(cx - 1, 0)) - keys.begin();
						const size_t b = std::upper_bound(keys.begin() + a, keys.end(), base | (uint64_t)(cx + 1)) - keys.begin();
						for (size_t j = a; j < b; j++)
							if (pts[j].id != id) H.offer(stat_d2(P, &pts[j].x), pts[j].id);
					}
				if (H.within(r2)) H.write(out_index + (size_t)id * k, out_dist_sq ? out_dist_sq + (size_t)id * k : nullptr); else open[e] = 1;
			}
		});
		next.clear();
		for (size_t e = 0; e < list.size(); e++) if (open[e]) next.push_back(list[e]);
		list.swap(next);
	}
	// the top level: every point is a candidate
	if (!list.empty())
		parallel_tasks(threads, (int)((list.size() + 255) / 256), [&](int t) {
			for (size_t e = (size_t)t * 256; e < std::min(list.size(), ((size_t)t + 1) * 256); e++) {
				const int32_t id = list[e];
				const float* P = xyz + 3 * (size_t)id;
				KeyHeap H(k);
				for (size_t j = 0; j < n; j++)
					if ((int32_t)j != id) H.offer(stat_d2(P, xyz + 3 * j), (int32_t)j);
				H.write(out_index + (size_t)id * k, out_dist_sq ? out_dist_sq + (size_t)id * k : nullptr);
			}
		});
}

}  // namespace

void knn_self_host(const float* xyz, size_t n, int32_t k, int32_t* out_index, float* out_dist_sq)
{
	if (!out_index) throw std::invalid_argument("goicp_knn_self_host: out_index must be non-null");
	float mn[3], mx[3];
	stat_check_cloud(xyz, n, mn, mx);
	knn_self_check_params(n, k);
	knn_self_rows(xyz, n, k, mn, mx, out_index, out_dist_sq);
}

void estimate_normals_host(const float* xyz, size_t n, int32_t k, const float* vp, float* out_normals, float* out_variation, int32_t* out_index)
{
	if (!out_normals) throw std::invalid_argument("goicp_estimate_normals_host: out_normals must be non-null");
	float mn[3], mx[3];
	stat_check_cloud(xyz, n, mn, mx);
	normals_check_params(n, k, vp);
	const int kk = k - 1;
	std::vector<int32_t> rows_own;
	if (!out_index) rows_own.resize(n * (size_t)kk);
	int32_t* rows = out_index ? out_index : rows_own.data();
	knn_self_rows(xyz, n, kk, mn, mx, rows, nullptr);
	const size_t chunk = 4096;
	parallel_tasks(n >= 65536 ? 8 : 1, (int)((n + chunk - 1) / chunk), [&](int t) {
		for (size_t i = (size_t)t * chunk; i < std::min(n, ((size_t)t + 1) * chunk); i++) {
			float var;
			normal_pca_point(xyz, (int)i, rows + i * (size_t)kk, kk, vp != nullptr, vp ? vp[0] : 0.f, vp ? vp[1] : 0.f, vp ? vp[2] : 0.f, out_normals + 3 * i, &var);
			if (out_variation) out_variation[i] = var;
		}
	});
}

// ---- FPFH descriptors and descriptor matching: what both paths share, and the host path ----
void fpfh_check_normals(const float* normals, size_t n)
{
	if (!normals) throw std::invalid_argument("goicp fpfh: the normals must be non-null");
	for (size_t i = 0; i < 3 * n; i++)
		if (!std::isfinite(normals[i])) throw std::invalid_argument("goicp fpfh: non-finite normal");
}

void match_check_descriptors(const float* q, size_t nq, const float* t, size_t nt)
{
	if (!q || !t || nq == 0 || nt == 0) throw std::invalid_argument("goicp match features: empty descriptor set");
	if (nq > (size_t)INT32_MAX / 8 || nt > (size_t)INT32_MAX / 8) throw std::invalid_argument("goicp match features: descriptor set too large");
	for (size_t i = 0; i < (size_t)kFpfhDim * nq; i++)
		if (!std::isfinite(q[i])) throw std::invalid_argument("goicp match features: non-finite query descriptor");
	for (size_t i = 0; i < (size_t)kFpfhDim * nt; i++)
		if (!std::isfinite(t[i])) throw std::invalid_argument("goicp match features: non-finite target descriptor");
}

void fpfh_host(const float* xyz, const float* normals, size_t n, int32_t k, float* out_fpfh, uint8_t* out_spfh_counts)
{
	if (!out_fpfh) throw std::invalid_argument("goicp_fpfh_host: out_fpfh must be non-null");
	float mn[3], mx[3];
	stat_check_cloud(xyz, n, mn, mx);
	knn_self_check_params(n, k);
	fpfh_check_normals(normals, n);
	std::vector<int32_t> rows(n * (size_t)k);
	std::vector<float> d2(n * (size_t)k);
	knn_self_rows(xyz, n, k, mn, mx, rows.data(), d2.data());
	std::vector<uint8_t> counts(n * (size_t)kFpfhDim, 0);
	const size_t chunk = 4096;
	const int threads = n >= 65536 ? 8 : 1, tasks = (int)((n + chunk - 1) / chunk);
	// the SPFH: the pair features of every point with its row, counted
	parallel_tasks(threads, tasks, [&](int t) {
		for (size_t i = (size_t)t * chunk; i < std::min(n, ((size_t)t + 1) * chunk); i++) {
			uint8_t* c = counts.data() + i * kFpfhDim;
			for (int j = 0; j < k; j++) {
				const size_t q = (size_t)rows[i * (size_t)k + j];
				int b[3];
				if (!fpfh::pair_bins(xyz + 3 * i, normals + 3 * i, xyz + 3 * q, normals + 3 * q, b)) continue;
				c[b[0]]++; c[kFpfhBins + b[1]]++; c[2 * kFpfhBins + b[2]]++;
			}
		}
	});
	// the FPFH: the neighbours' counts weighted by 1 / d2 in row order, each group of 11 scaled to 100, plus the point's own
	const double inc = 100.0 / (double)k;
	parallel_tasks(threads, tasks, [&](int t) {
		for (size_t i = (size_t)t * chunk; i < std::min(n, ((size_t)t + 1) * chunk); i++) {
			double a[kFpfhDim] = {};
			for (int j = 0; j < k; j++) {
				const float w2 = d2[i * (size_t)k + j];
				if (w2 == 0.f) continue;
				const double w = 1.0 / (double)w2;
				const uint8_t* c = counts.data() + (size_t)rows[i * (size_t)k + j] * kFpfhDim;
				for (int b = 0; b < kFpfhDim; b++) a[b] = a[b] + ((double)c[b] * inc) * w;
			}
			for (int g = 0; g < 3; g++) {
				double s = 0.0;
				for (int b = 0; b < kFpfhBins; b++) s = s + a[g * kFpfhBins + b];
				if (s > 0.0) {
					const double scale = 100.0 / s;
					for (int b = 0; b < kFpfhBins; b++) a[g * kFpfhBins + b] = a[g * kFpfhBins + b] * scale;
				}
			}
			for (int b = 0; b < kFpfhDim; b++) out_fpfh[i * kFpfhDim + b] = (float)(a[b] + (double)counts[i * kFpfhDim + b] * inc);
		}
	});
	if (out_spfh_counts) std::memcpy(out_spfh_counts, counts.data(), counts.size());
}

namespace {

// the two smallest keys (bits of d2) << 32 | t of every query of [a, b) over all targets
void match_rows(const float* q, size_t a, size_t b, const float* t, size_t nt, uint64_t* best, uint64_t* second)
{
	for (size_t i = a; i < b; i++) {
		const float* qi = q + i * kFpfhDim;
		uint64_t k1 = ~0ull, k2 = ~0ull;
		for (size_t j = 0; j < nt; j++) {
			const float* tj = t + j * kFpfhDim;
			float d2 = 0.f;
			for (int c = 0; c < kFpfhDim; c++) {
				const float d = qi[c] - tj[c];
				d2 = d2 + d * d;
			}
			uint32_t bits;
			std::memcpy(&bits, &d2, sizeof bits);
			const uint64_t key = ((uint64_t)bits << 32) | (uint32_t)j;
			if (key < k1) { k2 = k1; k1 = key; }
			else if (key < k2) k2 = key;
		}
		best[i] = k1;
		if (second) second[i] = k2;
	}
}

void match_all(const float* q, size_t nq, const float* t, size_t nt, std::vector<uint64_t>& best, std::vector<uint64_t>* second)
{
	best.resize(nq);
	if (second) second->resize(nq);
	const size_t chunk = std::max<size_t>(1, std::min<size_t>(256, (1u << 22) / (nt * kFpfhDim) + 1));
	const int threads = nq * nt >= ((size_t)1 << 22) ? 8 : 1;
	parallel_tasks(threads, (int)((nq + chunk - 1) / chunk), [&](int task) {
		match_rows(q, (size_t)task * chunk, std::min(nq, ((size_t)task + 1) * chunk), t, nt, best.data(), second ? second->data() : nullptr);
	});
}

}  // namespace

void match_features_host(const float* q, size_t nq, const float* t, size_t nt, int32_t* out_index, float* out_d2, float* out_d2_second, uint8_t* out_mutual)
{
	if (!out_index || !out_d2 || !out_d2_second) throw std::invalid_argument("goicp_match_features_host: out_index, out_d2 and out_d2_second must be non-null");
	match_check_descriptors(q, nq, t, nt);
	std::vector<uint64_t> best, second, back;
	match_all(q, nq, t, nt, best, &second);
	if (out_mutual) match_all(t, nt, q, nq, back, nullptr);
	auto d2_of = [](uint64_t key) {
		const uint32_t bits = (uint32_t)(key >> 32);
		float d2;
		std::memcpy(&d2, &bits, sizeof d2);
		return d2;
	};
	for (size_t i = 0; i < nq; i++) {
		const uint32_t j = (uint32_t)(best[i] & 0xffffffffull);
		out_index[i] = (int32_t)j;
		out_d2[i] = d2_of(best[i]);
		out_d2_second[i] = second[i] == ~0ull ? INFINITY : d2_of(second[i]);
		if (out_mutual) out_mutual[i] = (uint32_t)(back[j] & 0xffffffffull) == (uint32_t)i ? 1 : 0;
	}
}

// ---- RANSAC plane segmentation: what both paths share, and the host path ----
void plane_check_cloud(const float* xyz, size_t n)
{
	if (!xyz || n == 0) throw std::invalid_argument("goicp plane: empty cloud");
	if (n > (size_t)INT32_MAX / 8) throw std::invalid_argument("goicp plane: cloud too large");
	for (size_t i = 0; i < 3 * n; i++)
		if (!std::isfinite(xyz[i])) throw std::invalid_argument("goicp plane: non-finite coordinate in the cloud");
}

PlaneSelect plane_check_select(float distance, int32_t iterations, int32_t refine, int32_t max_planes, int32_t min_inliers, uint64_t seed)
{
	if (!(distance > 0.f) || !std::isfinite(distance)) throw std::invalid_argument("goicp plane: the distance must be positive and finite");
	if (iterations < 0 || iterations > kPlaneMaxIterations) throw std::invalid_argument("goicp plane: iterations must be in 0..65536 (0 = 1000)");
	if (refine < 0 || refine > 1) throw std::invalid_argument("goicp plane: refine must be 0 or 1");
	if (max_planes < 0 || max_planes > kPlaneMaxPlanes) throw std::invalid_argument("goicp plane: max_planes must be in 0..8 (0 = 1)");
	if (min_inliers < 0) throw std::invalid_argument("goicp plane: min_inliers must not be negative");
	PlaneSelect s;
	s.distance = distance;
	s.iterations = iterations ? iterations : kPlaneDefaultIterations;
	s.refine = refine;
	s.max_planes = max_planes ? max_planes : 1;
	s.min_inliers = min_inliers;
	s.seed = seed;
	return s;
}

bool plane_refit(const unsigned long long words[kPlaneWords], const float mn[3], int e, float normal[3], float point[3])
{
	using namespace pca;
	const int sh = 31 - e;
	const unsigned long long m = words[0];
	if (m == 0) return false;
	const double md = (double)m, mm = md * md;
	// C_ab = (m P_ab - S_a S_b) 2^(-2 sh) / m^2, the integer formed exactly and rounded once
	static const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {0, 1, 2, 1, 2, 2};
	double c[6];
	for (int k = 0; k < 6; k++) {
		const __int128 P = (__int128)(((unsigned __int128)words[4 + k] << 32) + (unsigned __int128)words[10 + k]);
		const __int128 v = (__int128)m * P - (__int128)words[1 + pa[k]] * (__int128)words[1 + pb[k]];
		c[k] = std::ldexp((double)v, -2 * sh) / mm;
	}
	double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
	double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
	for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
		const bool r01 = rotate<0, 1>(A, V), r02 = rotate<0, 2>(A, V), r12 = rotate<1, 2>(A, V);
		if (!(r01 || r02 || r12)) break;
	}
	const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
	const int s1 = l1 < l0 ? 1 : 0;
	const int col = l2 < (s1 ? l1 : l0) ? 2 : s1;              // the smallest l, the lowest index on equal values
	const double v0 = V[0][col], v1 = V[1][col], v2 = V[2][col];
	const double len = root(add(add(mul(v0, v0), mul(v1, v1)), mul(v2, v2)));
	normal[0] = (float)div(v0, len); normal[1] = (float)div(v1, len); normal[2] = (float)div(v2, len);
	if (!plane::finite3(normal) || (normal[0] == 0.f && normal[1] == 0.f && normal[2] == 0.f)) return false;
	plane::sign(normal);
	for (int k = 0; k < 3; k++) point[k] = (float)((double)mn[k] + std::ldexp((double)words[1 + k] / md, -sh));
	return true;
}

namespace {

struct PlaneHyp { float a[3], n[3]; bool ok; };

// the count of one plane over a cloud
int32_t plane_count(const float* xyz, size_t n, const float a[3], const float nr[3], float distance)
{
	int32_t cnt = 0;
	for (size_t i = 0; i < n; i++) cnt += plane::inlier(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], a[0], a[1], a[2], nr[0], nr[1], nr[2], distance) ? 1 : 0;
	return cnt;
}

}  // namespace

// the rounds of the header, on the remaining cloud `cur` (input order) with its index map; threads over blocks of hypotheses (integer counts)
void segment_plane_host(const float* xyz, size_t n, const PlaneSelect& s, int32_t* out_label, float* out_xyz, int32_t* out_index, PlaneRecord* out_planes,
                        size_t* n_planes, size_t* m_out)
{
	std::vector<float> cur(xyz, xyz + 3 * n), nxt;
	std::vector<int32_t> map(n), nmap, label(n, -1);
	std::iota(map.begin(), map.end(), 0);
	const int T = s.iterations;
	std::vector<int32_t> counts((size_t)T);
	size_t found = 0;
	for (int p = 0; p < s.max_planes; p++) {
		const size_t np = cur.size() / 3;
		if (np < 3) break;
		const int chunk = 16, chunks = (T + chunk - 1) / chunk;
		parallel_tasks((uint64_t)np * (uint64_t)T >= (1ull << 20) ? 8 : 1, chunks, [&](int ch) {
			for (int t = ch * chunk; t < std::min(T, (ch + 1) * chunk); t++) {
				uint32_t a, b, c;
				float nr[3];
				plane::draw(s.seed, (uint64_t)p * (uint64_t)T + (uint64_t)t, (uint32_t)np, &a, &b, &c);
				const bool ok = plane::of_triple(&cur[3 * (size_t)a], &cur[3 * (size_t)b], &cur[3 * (size_t)c], nr);
				counts[(size_t)t] = ok ? plane_count(cur.data(), np, &cur[3 * (size_t)a], nr, s.distance) : 0;
			}
		});
		int best = 0;
		for (int t = 1; t < T; t++) if (counts[(size_t)t] > counts[(size_t)best]) best = t;   // ties: the smallest t
		if (counts[(size_t)best] < std::max(s.min_inliers, 3)) break;
		PlaneRecord rec;
		{
			uint32_t a, b, c;
			plane::draw(s.seed, (uint64_t)p * (uint64_t)T + (uint64_t)best, (uint32_t)np, &a, &b, &c);
			plane::of_triple(&cur[3 * (size_t)a], &cur[3 * (size_t)b], &cur[3 * (size_t)c], rec.normal);
			for (int k = 0; k < 3; k++) rec.point[k] = cur[3 * (size_t)a + k];
		}
		rec.inliers = counts[(size_t)best];
		rec.hypothesis = best;
		rec.refined = 0;
		if (s.refine) {
			float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, E = 0.f;
			for (size_t i = 0; i < np; i++)
				for (int k = 0; k < 3; k++) { mn[k] = std::min(mn[k], cur[3 * i + k]); mx[k] = std::max(mx[k], cur[3 * i + k]); }
			for (int k = 0; k < 3; k++) E = std::max(E, mx[k] - mn[k]);   // rounding is monotone: the largest offset is an axis' maximum's
			int e = 0;
			std::frexp(E, &e);
			unsigned long long w[kPlaneWords] = {};
			for (size_t i = 0; i < np; i++) {
				const float* x = &cur[3 * i];
				if (!plane::inlier(x[0], x[1], x[2], rec.point[0], rec.point[1], rec.point[2], rec.normal[0], rec.normal[1], rec.normal[2], s.distance)) continue;
				unsigned long long q[3];
				for (int k = 0; k < 3; k++) q[k] = (unsigned long long)std::llrint(std::ldexp((double)(x[k] - mn[k]), 31 - e));
				w[0]++;
				int j = 0;
				for (int ka = 0; ka < 3; ka++) {
					w[1 + ka] += q[ka];
					for (int kb = ka; kb < 3; kb++, j++) {
						const unsigned long long prod = q[ka] * q[kb];
						w[4 + j] += prod >> 32;
						w[10 + j] += prod & 0xffffffffull;
					}
				}
			}
			float rn[3], rp[3];
			if (plane_refit(w, mn, e, rn, rp)) {
				const int32_t cnt = plane_count(cur.data(), np, rp, rn, s.distance);
				if (cnt >= rec.inliers) {
					for (int k = 0; k < 3; k++) { rec.normal[k] = rn[k]; rec.point[k] = rp[k]; }
					rec.inliers = cnt;
					rec.refined = 1;
				}
			}
		}
		rec.d = plane::offset(rec.normal, rec.point);
		if (out_planes) out_planes[found] = rec;
		nxt.clear(); nmap.clear();
		for (size_t i = 0; i < np; i++) {
			const float* x = &cur[3 * i];
			if (plane::inlier(x[0], x[1], x[2], rec.point[0], rec.point[1], rec.point[2], rec.normal[0], rec.normal[1], rec.normal[2], s.distance)) {
				label[(size_t)map[i]] = (int32_t)found;
			} else {
				nxt.insert(nxt.end(), x, x + 3);
				nmap.push_back(map[i]);
			}
		}
		cur.swap(nxt); map.swap(nmap);
		found++;
	}
	if (out_label) std::memcpy(out_label, label.data(), sizeof(int32_t) * n);
	if (out_xyz && !cur.empty()) std::memcpy(out_xyz, cur.data(), sizeof(float) * cur.size());
	if (out_index && !map.empty()) std::memcpy(out_index, map.data(), sizeof(int32_t) * map.size());
	if (n_planes) *n_planes = found;
	if (m_out) *m_out = map.size();
}

// ---- RANSAC pose estimation from correspondences: what both paths share, and the host path ----
RansacPoseSelect ransac_pose_check_select(float distance, int32_t iterations, int32_t refine, int32_t max_poses, int32_t min_inliers, float edge_similarity,
                                          uint64_t seed)
{
	if (!(distance > 0.f) || !std::isfinite(distance)) throw std::invalid_argument("goicp ransac_pose: the distance must be positive and finite");
	if (iterations < 0 || iterations > kRansacPoseMaxIterations) throw std::invalid_argument("goicp ransac_pose: iterations must be in 0..1048576 (0 = 100000)");
	if (refine < 0 || refine > 1) throw std::invalid_argument("goicp ransac_pose: refine must be 0 or 1");
	if (max_poses < 0 || max_poses > kRansacPoseMaxPoses) throw std::invalid_argument("goicp ransac_pose: max_poses must be in 0..64 (0 = 1)");
	if (min_inliers < 0) throw std::invalid_argument("goicp ransac_pose: min_inliers must not be negative");
	if (!(edge_similarity >= 0.f && edge_similarity <= 1.f)) throw std::invalid_argument("goicp ransac_pose: edge_similarity must be 0 (off) or in (0, 1]");
	RansacPoseSelect s;
	s.distance = distance;
	s.iterations = iterations ? iterations : kRansacPoseDefaultIterations;
	s.refine = refine;
	s.max_poses = max_poses ? max_poses : 1;
	s.min_inliers = min_inliers;
	s.edge_similarity = edge_similarity;
	s.seed = seed;
	return s;
}

void ransac_pose_check_input(const float* src, size_t n_s, const float* tgt, size_t n_t, const int32_t* corr, size_t M)
{
	const size_t limit = (size_t)INT32_MAX / 8;
	if (!src || !tgt || !corr) throw std::invalid_argument("goicp ransac_pose: src, tgt and corr must be non-null");
	if (M < 3) throw std::invalid_argument("goicp ransac_pose: at least three correspondences are needed");
	if (n_s == 0 || n_t == 0 || M > limit || n_s > limit || n_t > limit) throw std::invalid_argument("goicp ransac_pose: a cloud is empty, or a size is too large");
	for (size_t j = 0; j < M; j++)
		if (corr[2 * j] < 0 || (size_t)corr[2 * j] >= n_s || corr[2 * j + 1] < 0 || (size_t)corr[2 * j + 1] >= n_t)
			throw std::invalid_argument("goicp ransac_pose: an index of corr is out of range");
	for (size_t i = 0; i < 3 * n_s; i++)
		if (!std::isfinite(src[i])) throw std::invalid_argument("goicp ransac_pose: non-finite coordinate in the source cloud");
	for (size_t i = 0; i < 3 * n_t; i++)
		if (!std::isfinite(tgt[i])) throw std::invalid_argument("goicp ransac_pose: non-finite coordinate in the target cloud");
}

// the voxel operator's frame over the points of one side that the correspondences name (side 0 source, 1 target)
void ransac_pose_frame(const float* xyz, const int32_t* corr, size_t M, int side, RansacPoseFrame* f)
{
	float mn[3] = {INFINITY, INFINITY, INFINITY}, E = 0.f;
	for (size_t j = 0; j < M; j++)
		for (int k = 0; k < 3; k++) mn[k] = std::min(mn[k], xyz[3 * (size_t)corr[2 * j + side] + k]);
	for (size_t j = 0; j < M; j++)
		for (int k = 0; k < 3; k++) E = std::max(E, xyz[3 * (size_t)corr[2 * j + side] + k] - mn[k]);
	for (int k = 0; k < 3; k++) f->mn[k] = mn[k];
	f->e = 0;
	std::frexp(E, &f->e);                                        // E < 2^e
}

bool ransac_pose_refit(const unsigned long long words[kRansacPoseWords], const RansacPoseFrame& fs, const RansacPoseFrame& ft, float R[9], float t[3])
{
	const int shs = 31 - fs.e, sht = 31 - ft.e;
	const unsigned long long m = words[0];
	if (m == 0) return false;
	const double md = (double)m, mm = md * md;
	// H_ab = (m P_ab - St_a Ss_b) 2^(-shs - sht) / m^2, the integer formed exactly and rounded once
	double H[3][3], cs[3], ct[3];
	for (int a = 0; a < 3; a++)
		for (int b = 0; b < 3; b++) {
			const __int128 P = (__int128)(((unsigned __int128)words[7 + 3 * a + b] << 32) + (unsigned __int128)words[16 + 3 * a + b]);
			const __int128 v = (__int128)m * P - (__int128)words[4 + a] * (__int128)words[1 + b];
			H[a][b] = std::ldexp((double)v, -shs - sht) / mm;
		}
	for (int k = 0; k < 3; k++) {
		cs[k] = (double)fs.mn[k] + std::ldexp((double)words[1 + k] / md, -shs);
		ct[k] = (double)ft.mn[k] + std::ldexp((double)words[4 + k] / md, -sht);
	}
	return pose::from_cross_covariance(H, cs, ct, R, t);
}

namespace {

struct PosePair { float s[3], m[3]; };

int32_t pose_count(const std::vector<PosePair>& pk, const float R[9], const float t[3], float d2max, uint8_t* mask)
{
	int32_t cnt = 0;
	for (size_t j = 0; j < pk.size(); j++) {
		const PosePair& p = pk[j];
		const bool in = pose::inlier(R, t, p.s[0], p.s[1], p.s[2], p.m[0], p.m[1], p.m[2], d2max);
		cnt += in ? 1 : 0;
		if (mask) mask[j] = in ? 1 : 0;
	}
	return cnt;
}

bool pose_of_hypothesis(const std::vector<PosePair>& pk, const RansacPoseSelect& s, int t, float R[9], float tr[3])
{
	uint32_t a, b, c;
	plane::draw(s.seed, (uint64_t)t, (uint32_t)pk.size(), &a, &b, &c);
	const PosePair &pa = pk[a], &pb = pk[b], &pc = pk[c];
	if (s.edge_similarity > 0.f && !pose::triple_ok(pa.s, pb.s, pc.s, pa.m, pb.m, pc.m, s.edge_similarity)) return false;
	return pose::of_triple(pa.s, pb.s, pc.s, pa.m, pb.m, pc.m, R, tr);
}

}  // namespace

// the header's definition on the host; threads over blocks of hypotheses (integer counts)
void ransac_pose_host(const float* src, const float* tgt, const int32_t* corr, size_t M, const RansacPoseSelect& s, RansacPoseRecord* out_poses, size_t* n_poses,
                      uint8_t* out_inlier)
{
	std::vector<PosePair> pk(M);
	for (size_t j = 0; j < M; j++)
		for (int k = 0; k < 3; k++) { pk[j].s[k] = src[3 * (size_t)corr[2 * j] + k]; pk[j].m[k] = tgt[3 * (size_t)corr[2 * j + 1] + k]; }
	const int T = s.iterations;
	const float d2max = s.distance * s.distance;
	std::vector<uint64_t> keys((size_t)T);
	const int chunk = 16, chunks = (T + chunk - 1) / chunk;
	parallel_tasks((uint64_t)M * (uint64_t)T >= (1ull << 20) ? 8 : 1, chunks, [&](int ch) {
		for (int t = ch * chunk; t < std::min(T, (ch + 1) * chunk); t++) {
			float R[9], tr[3];
			const int32_t cnt = pose_of_hypothesis(pk, s, t, R, tr) ? pose_count(pk, R, tr, d2max, nullptr) : 0;
			keys[(size_t)t] = ((uint64_t)(uint32_t)cnt << 32) | (uint64_t)(~(uint32_t)t);
		}
	});
	const size_t K = std::min<size_t>((size_t)s.max_poses, (size_t)T);
	std::partial_sort(keys.begin(), keys.begin() + (std::ptrdiff_t)K, keys.end(), std::greater<uint64_t>());
	size_t found = 0;
	for (; found < K; found++) {
		const int32_t cnt = (int32_t)(keys[found] >> 32);
		if (cnt < std::max(s.min_inliers, 3)) break;
		RansacPoseRecord& rec = out_poses[found];
		rec.hypothesis = (int32_t)(~(uint32_t)(keys[found] & 0xffffffffull));
		pose_of_hypothesis(pk, s, rec.hypothesis, rec.R, rec.t);
		rec.inliers = cnt;
		rec.refined = 0;
	}
	if (s.refine && found > 0) {
		RansacPoseFrame fs, ft;
		ransac_pose_frame(src, corr, M, 0, &fs);
		ransac_pose_frame(tgt, corr, M, 1, &ft);
		for (size_t i = 0; i < found; i++) {
			RansacPoseRecord& rec = out_poses[i];
			unsigned long long w[kRansacPoseWords] = {};
			for (size_t j = 0; j < M; j++) {
				const PosePair& p = pk[j];
				if (!pose::inlier(rec.R, rec.t, p.s[0], p.s[1], p.s[2], p.m[0], p.m[1], p.m[2], d2max)) continue;
				unsigned long long qs[3], qt[3];
				for (int k = 0; k < 3; k++) {
					qs[k] = (unsigned long long)std::llrint(std::ldexp((double)(p.s[k] - fs.mn[k]), 31 - fs.e));
					qt[k] = (unsigned long long)std::llrint(std::ldexp((double)(p.m[k] - ft.mn[k]), 31 - ft.e));
				}
				w[0]++;
				for (int a = 0; a < 3; a++) {
					w[1 + a] += qs[a]; w[4 + a] += qt[a];
					for (int b = 0; b < 3; b++) {
						const unsigned long long prod = qt[a] * qs[b];
						w[7 + 3 * a + b] += prod >> 32;
						w[16 + 3 * a + b] += prod & 0xffffffffull;
					}
				}
			}
			float R[9], tr[3];
			if (ransac_pose_refit(w, fs, ft, R, tr)) {
				const int32_t cnt = pose_count(pk, R, tr, d2max, nullptr);
				if (cnt >= rec.inliers) {
					std::memcpy(rec.R, R, sizeof(R)); std::memcpy(rec.t, tr, sizeof(tr));
					rec.inliers = cnt;
					rec.refined = 1;
				}
			}
		}
	}
	if (out_inlier) {
		if (found > 0) pose_count(pk, out_poses[0].R, out_poses[0].t, d2max, out_inlier);
		else std::memset(out_inlier, 0, M);
	}
	*n_poses = found;
}

void select_matches_host(const int32_t* index, const float* d2, const float* d2_second, const uint8_t* mutual, size_t n_q, float ratio, int32_t require_mutual,
                         int32_t* out_corr, size_t* M)
{
	if (!index || !d2 || !d2_second || !out_corr || !M) throw std::invalid_argument("goicp_select_matches: index, d2, d2_second, out_corr and M must be non-null");
	if (n_q == 0 || n_q > (size_t)INT32_MAX / 8) throw std::invalid_argument("goicp_select_matches: n_q must be in 1..goicp_create's limit");
	if (!(ratio >= 0.f) || !std::isfinite(ratio)) throw std::invalid_argument("goicp_select_matches: the ratio must be 0 (no test) or positive and finite");
	if (require_mutual < 0 || require_mutual > 1) throw std::invalid_argument("goicp_select_matches: require_mutual must be 0 or 1");
	if (require_mutual && !mutual) throw std::invalid_argument("goicp_select_matches: require_mutual needs the mutual flags");
	const float rr = ratio * ratio;
	size_t m = 0;
	for (size_t q = 0; q < n_q; q++) {
		if (require_mutual && !mutual[q]) continue;
		if (ratio != 0.f && !(d2[q] <= rr * d2_second[q])) continue;
		out_corr[2 * m] = (int32_t)q; out_corr[2 * m + 1] = index[q];
		m++;
	}
	*M = m;
}

}  // namespace goicp
