// Device-side construction of the 64-ary box hierarchy: Morton codes -> rocPRIM radix
// sort -> balanced runs of <= 16 points per leaf -> bottom-up box unions.  Same KdDesc layout as the
// host median-split build (kdtree.cpp); the walk is exact for any hierarchy, only its speed depends
// on how tight the boxes are (median splits are tighter; this build is for clouds of 10^5..10^6+
// points, where the host build costs tenths of a second).
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "device.hpp"

namespace goicp {

// The device temporaries of one launcher.  get() allocates and keeps the pointer; the destructor frees what was allocated on every exit
// path -- not what the launcher's locals name by then, so swapping two of them (lists / lists2, cur / nxt) is harmless.  Nothing here
// throws: the launchers return hipError_t
class Temps {
public:
	Temps() = default;
	Temps(const Temps&) = delete;
	Temps& operator=(const Temps&) = delete;
	~Temps() { for (int i = 0; i < count_; i++) hipFree(owned_[i]); }
	hipError_t get_bytes(void*& p, size_t bytes)
	{
		if (count_ == kMax) return hipErrorOutOfMemory;
		const hipError_t e = hipMalloc(&p, bytes);
		if (e == hipSuccess) owned_[count_++] = p;
		return e;
	}
	template <class T> hipError_t get(T*& p, size_t n)
	{
		void* v = nullptr;
		const hipError_t e = get_bytes(v, sizeof(T) * n);
		p = static_cast<T*>(v);
		return e;
	}

private:
	static constexpr int kMax = 16;                              // the statistical filter's 14 are the most
	void* owned_[kMax];
	int count_ = 0;
};
#define KD_TRY(x) do { const hipError_t kd_try_e = (x); if (kd_try_e != hipSuccess) return kd_try_e; } while (0)

// the end of a launcher's device work: ev_end (may be null), then the stream drains -- the launcher's temporaries are in use until then
static hipError_t end_and_drain(hipEvent_t ev_end, hipStream_t stream)
{
	if (ev_end) KD_TRY(hipEventRecord(ev_end, stream));
	return hipStreamSynchronize(stream);
}

// a 64-bit shuffle is two 32-bit ones
template <class F> __device__ __forceinline__ unsigned long long shfl64_halves(unsigned long long v, F f)
{
	const int lo = f((int)(unsigned)(v & 0xffffffffull));
	const int hi = f((int)(unsigned)(v >> 32));
	return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) { return shfl64_halves(v, [=](int w) { return __shfl(w, src, 64); }); }
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int off) { return shfl64_halves(v, [=](int w) { return __shfl_up(w, off, 64); }); }
__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int off) { return shfl64_halves(v, [=](int w) { return __shfl_xor(w, off, 64); }); }

__device__ __forceinline__ unsigned spread10(unsigned x)
{
	x &= 0x3ffu;
	x = (x ^ (x << 16)) & 0xff0000ffu;
	x = (x ^ (x << 8)) & 0x0300f00fu;
	x = (x ^ (x << 4)) & 0x030c30c3u;
	x = (x ^ (x << 2)) & 0x09249249u;
	return x;
}

__global__ void kd_morton_kernel(const float* __restrict__ xyz, int M, float mnx, float mny, float mnz, float inv_ext,
                                 unsigned* __restrict__ keys, int* __restrict__ vals)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= M) return;
	const float fx = (xyz[3 * i] - mnx) * inv_ext, fy = (xyz[3 * i + 1] - mny) * inv_ext, fz = (xyz[3 * i + 2] - mnz) * inv_ext;
	const unsigned qx = (unsigned)fminf(1023.f, fmaxf(0.f, fx * 1024.f));
	const unsigned qy = (unsigned)fminf(1023.f, fmaxf(0.f, fy * 1024.f));
	const unsigned qz = (unsigned)fminf(1023.f, fmaxf(0.f, fz * 1024.f));
	keys[i] = spread10(qx) | (spread10(qy) << 1) | (spread10(qz) << 2);
	vals[i] = i;
}

// one thread per leaf: leaf f owns the sorted points [f*M/L, (f+1)*M/L) (<= kLeafSlots of them)
__global__ void kd_leaves_kernel(const float* __restrict__ xyz, const int* __restrict__ order, int M, int L,
                                 float4* __restrict__ pts, float* __restrict__ last_level_boxes)
{
	const int f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f >= L) return;
	const long long a = (long long)f * M / L, b = (long long)(f + 1) * M / L;
	float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	for (int s = 0; s < kLeafSlots; s++) {
		float4 p = make_float4(INFINITY, INFINITY, INFINITY, __int_as_float(INT_MAX));
		if (a + s < b) {
			const int id = order[a + s];
			p = make_float4(xyz[3 * id], xyz[3 * id + 1], xyz[3 * id + 2], __int_as_float(id));
			lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
			hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
		}
		pts[(size_t)f * kLeafSlots + s] = p;
	}
	float* rec = last_level_boxes + (size_t)(f >> 6) * 384;
	const int c = f & 63;
	for (int k = 0; k < 3; k++) { rec[64 * k + c] = lo[k]; rec[192 + 64 * k + c] = hi[k]; }
}

// child c of group g on `upper` = union of the 64 children of group 64g+c on `lower`
__global__ void kd_level_kernel(const float* __restrict__ lower, float* __restrict__ upper, int upper_children)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= upper_children) return;
	const float* src = lower + (size_t)t * 384;
	float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	for (int c = 0; c < 64; c++)
		for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], src[64 * k + c]); hi[k] = fmaxf(hi[k], src[192 + 64 * k + c]); }
	float* rec = upper + (size_t)(t >> 6) * 384;
	for (int k = 0; k < 3; k++) { rec[64 * k + (t & 63)] = lo[k]; rec[192 + 64 * k + (t & 63)] = hi[k]; }
}

// boxes[l] must hold 64^l * 384 floats, pts kLeafSlots * 64^K float4; d_xyz = the M target points on the device
hipError_t launch_kd_build(const float* d_xyz, int M, int K, const float mn[3], float ext, float* const boxes[kMaxLevels],
                           float4* pts, hipStream_t stream)
{
	const int L = 1 << (6 * K);
	unsigned *keys = nullptr, *keys2 = nullptr;
	int *vals = nullptr, *vals2 = nullptr;
	void* tmp = nullptr;
	size_t tmp_bytes = 0;
	Temps t;
	KD_TRY(t.get(keys, M));
	KD_TRY(t.get(keys2, M));
	KD_TRY(t.get(vals, M));
	KD_TRY(t.get(vals2, M));
	hipLaunchKernelGGL(kd_morton_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, d_xyz, M, mn[0], mn[1], mn[2],
	                   ext > 0.f ? 1.f / ext : 0.f, keys, vals);
	KD_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, keys2, vals, vals2, (size_t)M, 0, 30, stream));
	KD_TRY(t.get_bytes(tmp, tmp_bytes ? tmp_bytes : 16));
	KD_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys2, vals, vals2, (size_t)M, 0, 30, stream));
	hipLaunchKernelGGL(kd_leaves_kernel, dim3((L + 255) / 256), dim3(256), 0, stream, d_xyz, vals2, M, L, pts, boxes[K - 1]);
	for (int l = K - 2; l >= 0; l--) {
		const int upper_children = 1 << (6 * (l + 1));
		hipLaunchKernelGGL(kd_level_kernel, dim3((upper_children + 255) / 256), dim3(256), 0, stream, boxes[l + 1], boxes[l], upper_children);
	}
	KD_TRY(hipStreamSynchronize(stream));        // the temporaries are in use until here
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Source order on the device (Params::morton_sort; host twin: source_order_host, kdtree.cpp).
//
// Mode 2, the k-d order.  The host recursion splits a run at the source_order_left(n)-th element of the order (coordinate on the longest
// axis of the run's bounding box, index) and recurses down to single points.  The size of the left part depends on the run's length only,
// the comparator is a total order and the recursion ends at single points, so the permutation is unique -- and every level of the
// recursion can be done for all runs at once:
//   * the point ids are sorted once per axis by (key(coordinate), id) -- a stable radix sort of ascending ids;
//   * invariant: inside every run, each of the three lists holds the run's points in that axis' order.  So the run's bounding box is the
//     first and the last element of each list, and the left part is the first nl entries of the longest axis' list;
//   * a level flags the ids of the left parts, then stable-partitions all three lists inside every run (rank = exclusive scan of the
//     flags minus its value at the run's start), which keeps the invariant for both halves; the chosen axis' list comes out unchanged;
//   * the run bounds live per position in device arrays and are rewritten by the level's own kernel; the number of levels is a function
//     of N alone (the host counts it), so the loop has no round trip at all.
// After the last level every run is a single point and any list is the permutation.
// ------------------------------------------------------------------------------------------------
// order-preserving key of a float; -0 ties with +0 as in the host's fa == fb
__device__ __forceinline__ unsigned so_key(float f)
{
	unsigned b = __float_as_uint(f);
	if (b == 0x80000000u) b = 0u;
	return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ void so_axis_keys_kernel(const float* __restrict__ xyz, int n, int axis, unsigned* __restrict__ keys, int* __restrict__ ids)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	keys[i] = so_key(xyz[3 * (size_t)i + axis]);
	ids[i] = i;
}

// the host's 30-bit code: (s - mn) / ext, * 1024.f, clamp, cast -- IEEE division, nothing fused (the file is built with -ffp-contract=off)
__global__ void so_morton_kernel(const float* __restrict__ xyz, int n, float mnx, float mny, float mnz, float ext,
                                 unsigned* __restrict__ keys, int* __restrict__ ids)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float fx = __fdiv_rn(xyz[3 * (size_t)i] - mnx, ext), fy = __fdiv_rn(xyz[3 * (size_t)i + 1] - mny, ext), fz = __fdiv_rn(xyz[3 * (size_t)i + 2] - mnz, ext);
	const unsigned qx = (unsigned)fminf(1023.f, fmaxf(0.f, fx * 1024.f));
	const unsigned qy = (unsigned)fminf(1023.f, fmaxf(0.f, fy * 1024.f));
	const unsigned qz = (unsigned)fminf(1023.f, fmaxf(0.f, fz * 1024.f));
	keys[i] = spread10(qx) | (spread10(qy) << 1) | (spread10(qz) << 2);
	ids[i] = i;
}

__global__ void so_iota_kernel(int* __restrict__ v, int n)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) v[i] = i;
}

__global__ void so_root_kernel(int* __restrict__ lo, int* __restrict__ hi, int n)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) { lo[i] = 0; hi[i] = n; }
}

// one thread per POSITION i: its run [lo, hi), the run's longest axis (the host's float expression, first axis wins a tie), the flag of the
// id at position i of that axis' list (1 = left part), and the bounds of the half position i belongs to from the next level on
__global__ void so_flag_kernel(const float* __restrict__ xyz, const int* __restrict__ lists, int n, const int* __restrict__ lo, const int* __restrict__ hi,
                               int* __restrict__ lo2, int* __restrict__ hi2, unsigned char* __restrict__ flag)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int a = lo[i], b = hi[i], len = b - a;
	if (len <= 1) {
		flag[lists[i]] = 1;
		lo2[i] = a; hi2[i] = b;
		return;
	}
	float ext[3];
	for (int k = 0; k < 3; k++) {
		const int* L = lists + (size_t)k * n;
		ext[k] = xyz[3 * (size_t)L[b - 1] + k] - xyz[3 * (size_t)L[a] + k];
	}
	int ax = 0;
	for (int k = 1; k < 3; k++) if (ext[k] > ext[ax]) ax = k;
	const int nl = source_order_left(len);
	const bool left = i - a < nl;
	flag[lists[(size_t)ax * n + i]] = left ? 1 : 0;
	lo2[i] = left ? a : a + nl;
	hi2[i] = left ? a + nl : b;
}

struct SoFlagOf {
	const int* lists;
	const unsigned char* flag;
	__device__ int operator()(int j) const { return (int)flag[lists[j]]; }
};

// one thread per list entry j = k n + i: the stable partition of list k inside the run of position i.  scan = exclusive scan of the
// flags over all 3 n entries; its value at the run's start is subtracted, so the lists may share one scan
__global__ void so_partition_kernel(const int* __restrict__ lists, int* __restrict__ lists2, int n, const int* __restrict__ lo, const int* __restrict__ hi,
                                    const unsigned char* __restrict__ flag, const int* __restrict__ scan)
{
	const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= 3LL * n) return;
	const int k = (int)(j / n), i = (int)(j - (long long)k * n);
	const int a = lo[i], len = hi[i] - a;
	const int nl = source_order_left(len);
	const int id = lists[j];
	const int r = scan[j] - scan[(size_t)k * n + a];          // flagged entries of this run before position i
	const int pos = flag[id] ? a + r : a + nl + (i - a - r);
	if (pos >= a && pos < a + len) lists2[(size_t)k * n + pos] = id;
}

__global__ void so_gather_kernel(const float* __restrict__ xyz, const int* __restrict__ perm, int n, float4* __restrict__ out)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const size_t id = (size_t)perm[i];
	const float x = xyz[3 * id], y = xyz[3 * id + 1], z = xyz[3 * id + 2];
	out[i] = make_float4(x, y, z, sqrtf(x * x + y * y + z * z));   // normData, jly_goicp.cpp:145
}

// levels of the k-d order's recursion for n points: the lengths at a level are few distinct values, all functions of n
static int source_order_levels(int n)
{
	std::vector<int> cur{n};
	int levels = 0;
	while (cur.back() > 1) {
		std::vector<int> next;
		for (int v : cur) {
			const int nl = source_order_left(v);
			next.push_back(nl);
			if (v > 1) next.push_back(v - nl);
		}
		std::sort(next.begin(), next.end());
		next.erase(std::unique(next.begin(), next.end()), next.end());
		cur.swap(next);
		levels++;
	}
	return levels;
}

hipError_t launch_source_order(const float* d_xyz, int n, int mode, const float mn[3], float ext, int32_t* d_perm, hipStream_t stream)
{
	if (n <= 0) return hipErrorInvalidValue;
	const dim3 blk(256), grd((n + 255) / 256);
	if (mode <= 0) {
		hipLaunchKernelGGL(so_iota_kernel, grd, blk, 0, stream, d_perm, n);
		KD_TRY(hipGetLastError());
		return hipStreamSynchronize(stream);
	}
	unsigned *keys = nullptr, *keys2 = nullptr;
	int *ids = nullptr, *lists = nullptr, *lists2 = nullptr, *scan = nullptr, *seg = nullptr;
	unsigned char* flag = nullptr;
	void* tmp = nullptr;
	Temps t;
	const size_t N = (size_t)n;
	KD_TRY(t.get(keys, N));
	KD_TRY(t.get(keys2, N));
	KD_TRY(t.get(ids, N));
	size_t sort_bytes = 0, scan_bytes = 0;
	if (mode == 1) {
		hipLaunchKernelGGL(so_morton_kernel, grd, blk, 0, stream, d_xyz, n, mn[0], mn[1], mn[2], ext, keys, ids);
		KD_TRY(hipGetLastError());
		KD_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, keys2, ids, d_perm, N, 0, 30, stream));
		KD_TRY(t.get_bytes(tmp, sort_bytes ? sort_bytes : 16));
		KD_TRY(rocprim::radix_sort_pairs(tmp, sort_bytes, keys, keys2, ids, d_perm, N, 0, 30, stream));
		return hipStreamSynchronize(stream);         // the temporaries are in use until here
	}
	const int levels = source_order_levels(n);
	KD_TRY(t.get(lists, 3 * N));
	if (levels > 0) {
		KD_TRY(t.get(lists2, 3 * N));
		KD_TRY(t.get(scan, 3 * N));
		KD_TRY(t.get(seg, 4 * N));
		KD_TRY(t.get(flag, N));
	}
	auto flags_of = [&](const int* l) { return rocprim::make_transform_iterator(rocprim::counting_iterator<int>(0), SoFlagOf{l, flag}); };
	KD_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, keys2, ids, lists, N, 0, 32, stream));
	if (levels > 0) KD_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, flags_of(lists), scan, 0, 3 * N, rocprim::plus<int>(), stream));
	const size_t tmp_bytes = std::max<size_t>(std::max(sort_bytes, scan_bytes), 16);
	KD_TRY(t.get_bytes(tmp, tmp_bytes));
	for (int k = 0; k < 3; k++) {
		hipLaunchKernelGGL(so_axis_keys_kernel, grd, blk, 0, stream, d_xyz, n, k, keys, ids);
		KD_TRY(hipGetLastError());
		size_t bytes = sort_bytes;
		KD_TRY(rocprim::radix_sort_pairs(tmp, bytes, keys, keys2, ids, lists + (size_t)k * N, N, 0, 32, stream));
	}
	if (levels > 0) {
		int *lo = seg, *hi = seg + N, *lo2 = seg + 2 * N, *hi2 = seg + 3 * N;
		hipLaunchKernelGGL(so_root_kernel, grd, blk, 0, stream, lo, hi, n);
		KD_TRY(hipGetLastError());
		const dim3 grd3((unsigned)((3 * N + 255) / 256));
		for (int l = 0; l < levels; l++) {
			hipLaunchKernelGGL(so_flag_kernel, grd, blk, 0, stream, d_xyz, lists, n, lo, hi, lo2, hi2, flag);
			KD_TRY(hipGetLastError());
			size_t bytes = scan_bytes;
			KD_TRY(rocprim::exclusive_scan(tmp, bytes, flags_of(lists), scan, 0, 3 * N, rocprim::plus<int>(), stream));
			hipLaunchKernelGGL(so_partition_kernel, grd3, blk, 0, stream, lists, lists2, n, lo, hi, flag, scan);
			KD_TRY(hipGetLastError());
			std::swap(lists, lists2);
			std::swap(lo, lo2);
			std::swap(hi, hi2);
		}
	}
	KD_TRY(hipMemcpyAsync(d_perm, lists, sizeof(int) * N, hipMemcpyDeviceToDevice, stream));
	return hipStreamSynchronize(stream);             // the temporaries are in use until here
}

hipError_t launch_source_gather(const float* d_xyz, const int32_t* d_perm, int n, float4* d_src, hipStream_t stream)
{
	hipLaunchKernelGGL(so_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_xyz, d_perm, n, d_src);
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Voxel-grid downsampling on the device (host twin: voxel_downsample_host, kdtree.cpp): one centroid per occupied cell, cells in
// ascending key order.  rocPRIM's are the radix sort of (key, id) and the inclusive scan of the head flags (the cell index of every sorted
// position); ours are the key kernel, the segmented sum and the finishing kernel.  The sums are exact 64-bit integers -- the term of a
// coordinate is llrint(ldexp(d, s)), VoxelFrame::s chosen so that n terms stay below 2^62 -- so the order of addition cannot matter and the
// pieces of a cell that spans several waves may arrive by atomicAdd in any order.
// ------------------------------------------------------------------------------------------------
// the cell of an offset d >= 0 from the frame's minimum: IEEE division, as the host's (int)floorf(d / v)
__device__ __forceinline__ unsigned long long vx_cell(float d, float v) { return (unsigned long long)(int)floorf(__fdiv_rn(d, v)); }

__global__ void vx_key_kernel(const float* __restrict__ xyz, int n, float mnx, float mny, float mnz, float v, unsigned long long* __restrict__ keys,
                              int* __restrict__ ids)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float dx = xyz[3 * (size_t)i] - mnx, dy = xyz[3 * (size_t)i + 1] - mny, dz = xyz[3 * (size_t)i + 2] - mnz;
	keys[i] = vx_cell(dx, v) | (vx_cell(dy, v) << 21) | (vx_cell(dz, v) << 42);
	ids[i] = i;
}

struct VxHeadOf {
	const unsigned long long* keys;
	__device__ int operator()(int i) const { return (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0; }
};

// The sorted cell grid of a VoxelFrame, which every grid operator starts from: the key of every point (vx_key_kernel), rocPRIM's radix sort
// of (key, id) over the frame's used key bits -- stable, and the ids start ascending, so the ids of a cell ascend -- and, for the operators
// that walk tiles, the gather into sorted 16-byte records
struct __align__(16) RorPt { float x, y, z; int id; };

__global__ void ror_gather_kernel(const float* __restrict__ xyz, const int* __restrict__ ids, int n, RorPt* __restrict__ pts)
{
	const int s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const int id = ids[s];
	pts[s] = RorPt{xyz[3 * (size_t)id], xyz[3 * (size_t)id + 1], xyz[3 * (size_t)id + 2], id};
}

struct CellGrid {
	unsigned long long *keys = nullptr, *sorted_keys = nullptr;  // by input index; ascending
	int *ids = nullptr, *order = nullptr;                        // 0..n-1; the input index of every sorted position
	RorPt* pts = nullptr;                                        // the records in sorted order (not allocated for the voxel operator)
	hipError_t alloc(Temps& t, size_t N, bool records)
	{
		KD_TRY(t.get(keys, N));
		KD_TRY(t.get(sorted_keys, N));
		KD_TRY(t.get(ids, N));
		KD_TRY(t.get(order, N));
		if (records) KD_TRY(t.get(pts, N));
		return hipSuccess;
	}
};

static unsigned grid_end_bit(const VoxelFrame& f) { return (unsigned)std::min(std::max(f.key_bits, 1), 63); }

// bytes = the sort's temporary storage for the largest of `count` frames
static hipError_t grid_sort_bytes(const CellGrid& g, size_t N, const VoxelFrame* frames, int count, size_t& bytes, hipStream_t stream)
{
	bytes = 0;
	for (int L = 0; L < count; L++) {
		size_t b = 0;
		KD_TRY(rocprim::radix_sort_pairs(nullptr, b, g.keys, g.sorted_keys, g.ids, g.order, N, 0, grid_end_bit(frames[L]), stream));
		bytes = std::max(bytes, b);
	}
	return hipSuccess;
}

// keys and order of frame f; tmp holds sort_bytes as grid_sort_bytes reported them
static hipError_t grid_sort(const float* d_xyz, int n, const VoxelFrame& f, const CellGrid& g, void* tmp, size_t sort_bytes, hipStream_t stream)
{
	hipLaunchKernelGGL(vx_key_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_xyz, n, f.mn[0], f.mn[1], f.mn[2], f.voxel, g.keys, g.ids);
	KD_TRY(hipGetLastError());
	return rocprim::radix_sort_pairs(tmp, sort_bytes, g.keys, g.sorted_keys, g.ids, g.order, (size_t)n, 0, grid_end_bit(f), stream);
}

// grid_sort and the records
static hipError_t grid_build(const float* d_xyz, int n, const VoxelFrame& f, const CellGrid& g, void* tmp, size_t sort_bytes, hipStream_t stream)
{
	KD_TRY(grid_sort(d_xyz, n, f, g, tmp, sort_bytes, stream));
	hipLaunchKernelGGL(ror_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_xyz, g.order, n, g.pts);
	return hipGetLastError();
}

// One thread per SORTED position i (blocks of 256 = 4 waves of 64 consecutive positions).  cell1[i] = 1 + the cell index of position i (the
// inclusive scan of the head flags).  Inside a wave, a segmented inclusive scan over the head flags: a lane adds the value 2^k lanes below
// while that lane is still inside its own segment.  The last lane of every segment piece holds the piece's sums.  A segment that opens and
// closes inside the wave is stored plainly (nobody else writes its cell); a piece of a segment cut by a wave edge -- at most the first and
// the last piece of a wave -- is added to the zeroed accumulators with 64-bit atomicAdd.  acc: 4 words per cell (three sums, the count);
// first_id[cell]: the id of the cell's first sorted point (the one a singleton cell returns)
__global__ void __launch_bounds__(256) vx_segsum_kernel(const float* __restrict__ xyz, const int* __restrict__ ids, const int* __restrict__ cell1, int n,
                                                        float mnx, float mny, float mnz, int s, unsigned long long* __restrict__ acc,
                                                        int* __restrict__ first_id)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	const int lane = threadIdx.x & 63;
	const bool valid = i < n;
	long long t0 = 0, t1 = 0, t2 = 0;
	int cnt = 0, c1 = 0;
	bool head = true;                                          // a lane past the end closes the segment below it
	if (valid) {
		const int id = ids[i];
		c1 = cell1[i];
		head = i == 0 || cell1[i - 1] != c1;
		const float dx = xyz[3 * (size_t)id] - mnx, dy = xyz[3 * (size_t)id + 1] - mny, dz = xyz[3 * (size_t)id + 2] - mnz;
		t0 = llrint(ldexp((double)dx, s)); t1 = llrint(ldexp((double)dy, s)); t2 = llrint(ldexp((double)dz, s));
		cnt = 1;
		if (head) first_id[c1 - 1] = id;
	}
	const unsigned long long heads = __ballot(head);
	const unsigned long long below = heads & (~0ull >> (63 - lane));        // the heads at or below this lane
	const int start = below ? 63 - __clzll(below) : 0;          // first lane of this lane's piece
	const int reach = lane - start;
	for (int off = 1; off < 64; off <<= 1) {
		const long long u0 = (long long)shfl_up64((unsigned long long)t0, off), u1 = (long long)shfl_up64((unsigned long long)t1, off),
		                u2 = (long long)shfl_up64((unsigned long long)t2, off);
		const int uc = __shfl_up(cnt, off, 64);
		if (off <= reach) { t0 += u0; t1 += u1; t2 += u2; cnt += uc; }
	}
	if (!valid) return;
	const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
	if (!tail) return;
	const bool opened = below != 0ull;                          // the segment's head is in this wave
	const bool closed = lane < 63 || i == n - 1 || cell1[i + 1] != c1;
	unsigned long long* a = acc + 4 * (size_t)(c1 - 1);
	if (opened && closed) {
		a[0] = (unsigned long long)t0; a[1] = (unsigned long long)t1; a[2] = (unsigned long long)t2; a[3] = (unsigned long long)cnt;
	} else {
		atomicAdd(a, (unsigned long long)t0); atomicAdd(a + 1, (unsigned long long)t1); atomicAdd(a + 2, (unsigned long long)t2);
		atomicAdd(a + 3, (unsigned long long)cnt);
	}
}

// one thread per cell: a singleton returns its point's own bits, any other cell (float)(mn + ldexp(S / count, -s)) in fp64
__global__ void vx_finish_kernel(const float* __restrict__ xyz, const unsigned long long* __restrict__ acc, const int* __restrict__ first_id, int m,
                                 float mnx, float mny, float mnz, int s, float* __restrict__ out, int32_t* __restrict__ count)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= m) return;
	const unsigned long long* a = acc + 4 * (size_t)c;
	const long long cnt = (long long)a[3];
	float x, y, z;
	if (cnt == 1) {
		const size_t id = (size_t)first_id[c];
		x = xyz[3 * id]; y = xyz[3 * id + 1]; z = xyz[3 * id + 2];
	} else {
		x = (float)((double)mnx + ldexp((double)(long long)a[0] / (double)cnt, -s));
		y = (float)((double)mny + ldexp((double)(long long)a[1] / (double)cnt, -s));
		z = (float)((double)mnz + ldexp((double)(long long)a[2] / (double)cnt, -s));
	}
	out[3 * (size_t)c] = x; out[3 * (size_t)c + 1] = y; out[3 * (size_t)c + 2] = z;
	if (count) count[c] = (int32_t)cnt;
}

hipError_t launch_voxel_downsample(const float* d_xyz, int n, const VoxelFrame& f, float* d_out, int32_t* d_count, int* m_out, hipStream_t stream,
                                   hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (n <= 0 || !m_out) return hipErrorInvalidValue;
	const dim3 blk(256), grd((n + 255) / 256);
	unsigned long long* acc = nullptr;
	int *cell1 = nullptr, *first_id = nullptr;
	void* tmp = nullptr;
	Temps t;
	CellGrid g;
	const size_t N = (size_t)n;
	KD_TRY(g.alloc(t, N, false));
	KD_TRY(t.get(cell1, N));
	auto heads = rocprim::make_transform_iterator(rocprim::counting_iterator<int>(0), VxHeadOf{g.sorted_keys});
	size_t sort_bytes = 0, scan_bytes = 0;
	KD_TRY(grid_sort_bytes(g, N, &f, 1, sort_bytes, stream));
	KD_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, heads, cell1, N, rocprim::plus<int>(), stream));
	KD_TRY(t.get_bytes(tmp, std::max<size_t>(std::max(sort_bytes, scan_bytes), 16)));
	// ev_begin .. ev_end: the kernels, the 4-byte read-back of m and the two m-sized allocations; the n-sized allocations above and the
	// frees at the end are outside
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	KD_TRY(grid_sort(d_xyz, n, f, g, tmp, sort_bytes, stream));
	KD_TRY(rocprim::inclusive_scan(tmp, scan_bytes, heads, cell1, N, rocprim::plus<int>(), stream));
	int m = 0;                                                  // the last index + 1
	KD_TRY(hipMemcpyAsync(&m, cell1 + (N - 1), sizeof(int), hipMemcpyDeviceToHost, stream));
	KD_TRY(hipStreamSynchronize(stream));
	if (m < 1 || m > n) return hipErrorUnknown;
	KD_TRY(t.get(acc, 4 * (size_t)m));
	KD_TRY(t.get(first_id, (size_t)m));
	KD_TRY(hipMemsetAsync(acc, 0, sizeof(unsigned long long) * 4 * (size_t)m, stream));
	hipLaunchKernelGGL(vx_segsum_kernel, grd, blk, 0, stream, d_xyz, g.order, cell1, n, f.mn[0], f.mn[1], f.mn[2], f.s, acc, first_id);
	KD_TRY(hipGetLastError());
	hipLaunchKernelGGL(vx_finish_kernel, dim3((m + 255) / 256), blk, 0, stream, d_xyz, acc, first_id, m, f.mn[0], f.mn[1], f.mn[2], f.s, d_out, d_count);
	KD_TRY(hipGetLastError());
	*m_out = m;
	return end_and_drain(ev_end, stream);
}

// ------------------------------------------------------------------------------------------------
// Radius outlier removal on the device (host twin: radius_outlier_removal_host, kdtree.cpp).  A grid of pitch 1.03125 r only
// selects candidates -- any pair within r lies in cells that differ by at most one per axis -- and what counts is the float expression of
// the header, so every candidate set that covers the 27 cells gives the same bits.  rocPRIM's are the radix sort of (key, id) and the scan
// of the keep flags; ours are the key kernel (the voxel operator's), the gather into sorted 16-byte records, the count kernel and the
// compaction.
// ------------------------------------------------------------------------------------------------
constexpr int kRorBlock = 256;                                 // the span of sorted points a workgroup owns, and the LDS tile (4 KB)

// the first sorted position whose key is >= k (upper = false) or > k (upper = true); a negative k is below every key
__device__ __forceinline__ int ror_bound(const unsigned long long* __restrict__ keys, int n, long long k, bool upper)
{
	if (k < 0) return 0;
	int lo = 0, hi = n;
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		const unsigned long long v = keys[mid];
		if (upper ? v <= (unsigned long long)k : v < (unsigned long long)k) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// What the tile kernels of every grid operator share.  A workgroup owns a span of consecutive SORTED points first..last, keys Ka..Kb.  The
// cells around a point with key K are the 9 runs [K + D - 1, K + D + 1], D = dy 2^21 + dz 2^42, so all runs of the span lie in the 9
// intervals [Ka + D - 1, Kb + D + 1].  Lanes 0..8 find them by binary search, lane 0 makes them disjoint (D ascends, so both ends ascend:
// each interval starts no earlier than the one before it ends), so no candidate is offered twice.  A key of the intervals that is no
// neighbour cell -- a field that wrapped below zero, the cells between two rows -- is only a candidate that fails the distance test or the
// cull.  iv_lo / iv_hi: 9 words of LDS each; every lane of the workgroup calls, and the intervals are visible on return
__device__ __forceinline__ void grid_intervals(const unsigned long long* __restrict__ keys, int n, int first, int last, int* iv_lo, int* iv_hi)
{
	const int tid = threadIdx.x;
	if (tid < 9) {
		const long long D = (long long)(tid % 3 - 1) * (1ll << 21) + (long long)(tid / 3 - 1) * (1ll << 42);
		iv_lo[tid] = ror_bound(keys, n, (long long)keys[first] + D - 1, false);
		iv_hi[tid] = ror_bound(keys, n, (long long)keys[last] + D + 1, true);
	}
	__syncthreads();
	if (tid == 0)
		for (int o = 1; o < 9; o++) {
			iv_lo[o] = max(iv_lo[o], iv_hi[o - 1]);
			iv_hi[o] = max(iv_hi[o], iv_lo[o]);
		}
	__syncthreads();
}

// does one of the 9 runs of a point with key K meet a tile whose keys are ta..tb
__device__ __forceinline__ bool grid_tile_meets(long long K, long long ta, long long tb)
{
	bool need = false;
	for (int q = 0; q < 9; q++) {
		const long long c = K + (long long)(q % 3 - 1) * (1ll << 21) + (long long)(q / 3 - 1) * (1ll << 42);
		need = need || (c - 1 <= tb && c + 1 >= ta);
	}
	return need;
}

// A workgroup owns kRorBlock consecutive SORTED points and passes their candidate intervals (grid_intervals) through LDS in tiles of
// kRorBlock records; each lane tests its own point against every record of a tile, skips its own id and stops counting at min_neighbors.
// A wave skips a tile none of whose unsaturated lanes has a run that meets the tile's key range, and the workgroup leaves once every lane
// is saturated: a dense cell costs a lane min_neighbors hits, not the cell.  No workgroup waits on another.
__global__ void __launch_bounds__(kRorBlock) ror_count_kernel(const RorPt* __restrict__ pts, const unsigned long long* __restrict__ keys, int n, float r2,
                                                              int min_neighbors, int32_t* __restrict__ count, int* __restrict__ flag)
{
	__shared__ RorPt tile[kRorBlock];
	__shared__ int iv_lo[9], iv_hi[9];
	const int tid = threadIdx.x;
	const int first = blockIdx.x * kRorBlock, last = min(first + kRorBlock, n) - 1;
	const int s = first + tid;
	const bool valid = s < n;
	grid_intervals(keys, n, first, last, iv_lo, iv_hi);
	RorPt P{0.f, 0.f, 0.f, -1};
	long long K = 0;
	if (valid) { P = pts[s]; K = (long long)keys[s]; }
	int cnt = valid ? 0 : min_neighbors;                         // a lane past the end counts as saturated
	for (int o = 0; o < 9; o++) {
		const int lo = iv_lo[o], hi = iv_hi[o];
		for (int t0 = lo; t0 < hi; t0 += kRorBlock) {
			if (__syncthreads_and(cnt >= min_neighbors)) goto done;   // also: the previous tile has been read by everybody
			const int len = min(kRorBlock, hi - t0);
			if (tid < len) tile[tid] = pts[t0 + tid];
			__syncthreads();
			const bool need = cnt < min_neighbors && grid_tile_meets(K, (long long)keys[t0], (long long)keys[t0 + len - 1]);
			if (!__any(need)) continue;                          // wave-uniform; the next barrier is at the loop's head
			for (int j = 0; j < len; j++) {
				const RorPt Q = tile[j];
				const float dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
				const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
				if (d2 <= r2 && Q.id != P.id && cnt < min_neighbors) cnt++;
			}
		}
	}
done:
	if (valid) {
		count[P.id] = cnt;
		flag[P.id] = cnt == min_neighbors ? 1 : 0;
	}
}

// scan: the exclusive scan of the flags in input order (n + 1 entries, the last one is m)
__global__ void ror_compact_kernel(const float* __restrict__ xyz, const int* __restrict__ flag, const int* __restrict__ scan, int n,
                                   float* __restrict__ out, int32_t* __restrict__ index)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n || !flag[i]) return;
	const size_t d = (size_t)scan[i];
	out[3 * d] = xyz[3 * (size_t)i]; out[3 * d + 1] = xyz[3 * (size_t)i + 1]; out[3 * d + 2] = xyz[3 * (size_t)i + 2];
	if (index) index[d] = i;
}

// the same with the label column of the clustering
__global__ void cl_compact_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ label, const int* __restrict__ flag, const int* __restrict__ scan,
                                  int n, float* __restrict__ out, int32_t* __restrict__ index, int32_t* __restrict__ out_label)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n || !flag[i]) return;
	const size_t d = (size_t)scan[i];
	out[3 * d] = xyz[3 * (size_t)i]; out[3 * d + 1] = xyz[3 * (size_t)i + 1]; out[3 * d + 2] = xyz[3 * (size_t)i + 2];
	if (index) index[d] = i;
	if (out_label) out_label[d] = label[i];
}

// bytes = the temporary storage of compact_tail's scan
static hipError_t compact_scan_bytes(int* flag, int* scan, size_t N, size_t& bytes, hipStream_t stream)
{
	return rocprim::exclusive_scan(nullptr, bytes, flag, scan, 0, N + 1, rocprim::plus<int>(), stream);
}

// The tail of every filter.  flag: n + 1 ints whose first n a kernel on the stream has set (1 = keep, input order); scan: n + 1 ints; tmp
// holds scan_bytes.  Scans the flags, writes the kept points (with their labels when d_label is given) and enqueues the 4-byte read-back
// of scan[n] into *m, which holds the number kept, in 0..n, once the stream has drained (end_and_drain)
static hipError_t compact_tail(const float* d_xyz, int n, int* flag, int* scan, void* tmp, size_t scan_bytes, const int32_t* d_label, float* d_out,
                               int32_t* d_index, int32_t* d_out_label, int* m, hipStream_t stream)
{
	const dim3 blk(256), grd((n + 255) / 256);
	const size_t N = (size_t)n;
	KD_TRY(hipMemsetAsync(flag + N, 0, sizeof(int), stream));
	KD_TRY(rocprim::exclusive_scan(tmp, scan_bytes, flag, scan, 0, N + 1, rocprim::plus<int>(), stream));
	if (d_label) hipLaunchKernelGGL(cl_compact_kernel, grd, blk, 0, stream, d_xyz, d_label, flag, scan, n, d_out, d_index, d_out_label);
	else hipLaunchKernelGGL(ror_compact_kernel, grd, blk, 0, stream, d_xyz, flag, scan, n, d_out, d_index);
	KD_TRY(hipGetLastError());
	return hipMemcpyAsync(m, scan + N, sizeof(int), hipMemcpyDeviceToHost, stream);
}

hipError_t launch_radius_outlier_removal(const float* d_xyz, int n, const VoxelFrame& f, float r2, int min_neighbors, float* d_out, int32_t* d_index,
                                         int32_t* d_count, int* m_out, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (n <= 0 || !m_out || min_neighbors < 1) return hipErrorInvalidValue;
	int *flag = nullptr, *scan = nullptr, *cnt = nullptr;
	void* tmp = nullptr;
	Temps t;
	CellGrid g;
	const size_t N = (size_t)n;
	KD_TRY(g.alloc(t, N, true));
	KD_TRY(t.get(flag, N + 1));
	KD_TRY(t.get(scan, N + 1));
	if (!d_count) KD_TRY(t.get(cnt, N));
	size_t sort_bytes = 0, scan_bytes = 0;
	KD_TRY(grid_sort_bytes(g, N, &f, 1, sort_bytes, stream));
	KD_TRY(compact_scan_bytes(flag, scan, N, scan_bytes, stream));
	KD_TRY(t.get_bytes(tmp, std::max<size_t>(std::max(sort_bytes, scan_bytes), 16)));
	// ev_begin .. ev_end: the kernels and the 4-byte read-back of m; the allocations above and the frees at the end are outside
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	KD_TRY(grid_build(d_xyz, n, f, g, tmp, sort_bytes, stream));
	hipLaunchKernelGGL(ror_count_kernel, dim3((n + kRorBlock - 1) / kRorBlock), dim3(kRorBlock), 0, stream, g.pts, g.sorted_keys, n, r2, min_neighbors,
	                   d_count ? d_count : cnt, flag);
	KD_TRY(hipGetLastError());
	int m = -1;
	KD_TRY(compact_tail(d_xyz, n, flag, scan, tmp, scan_bytes, nullptr, d_out, d_index, nullptr, &m, stream));
	KD_TRY(end_and_drain(ev_end, stream));
	if (m < 0 || m > n) return hipErrorUnknown;
	*m_out = m;
	return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// Euclidean / DBSCAN clustering on the device (host twin: cluster_host, kdtree.cpp).  The radius filter's keys, sort, records and
// count kernel give the core flag; new are the component kernel (a single-pass lock-free union-find over the core pairs), the flatten
// kernel, the border kernel and the relabelling.  parent[] is indexed by input index and only ever holds parent[v] <= v: a hook puts the
// larger root under the smaller one and path halving replaces a parent by an ancestor, which is smaller still.  So every tree's root is
// its smallest index, and once every core pair within r has been united the root of a component is its smallest core index, whatever
// the order in which the workgroups ran.
// ------------------------------------------------------------------------------------------------
constexpr int kClBlock = 256;                                  // the count kernel's span and tile

__global__ void cl_init_kernel(int* __restrict__ parent, int* __restrict__ core, int n, int all_core)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	parent[i] = i;
	if (all_core) core[i] = 1;
}

// a parent word as the L2 holds it.  A stale value would do no harm either: a former parent of v stays an ancestor of v for good
__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree as far as this thread can see, with path halving.  Terminates: parent[v] <= v holds for every word at every moment
// and a non-root's parent is strictly smaller, so x strictly decreases from one iteration to the next, whatever other threads write
// meanwhile: at most x iterations.  atomicMin keeps every word monotone (g is an ancestor of x, and so is whatever the word holds)
__device__ __forceinline__ int cl_find(int* parent, int x)
{
	for (;;) {
		const int p = cl_load(parent + x);
		if (p == x) return x;
		const int g = cl_load(parent + p);
		if (g != p) atomicMin(parent + x, g);
		x = g;
	}
}

// Unite the trees of a and b: the larger root is hooked under the smaller by a compare-and-swap that succeeds only while the larger is
// still a root.  b < a cannot lie in a's tree when a is a root (its descendants are larger), so no hook closes a cycle.  Terminates: a
// failed swap returns the word's value old < a (somebody else hooked a), and the next round starts from old and from b' <= b < a, so
// max(a, b) strictly decreases from one round to the next: at most max(a, b) rounds.  Nothing here waits for another thread
__device__ __forceinline__ void cl_unite(int* parent, int a, int b)
{
	for (;;) {
		a = cl_find(parent, a);
		b = cl_find(parent, b);
		if (a == b) return;
		if (a < b) { const int t = a; a = b; b = t; }
		const int old = atomicCAS(parent + a, a, b);
		if (old == a) return;
		a = old;
	}
}

// The count kernel's shape: a workgroup owns kClBlock consecutive SORTED points and passes their candidate intervals through LDS in
// tiles, each record with its core flag.  A core lane unites its point with every core candidate within r that has a smaller index (each
// pair once).  The tile loops run over the intervals' lengths; the loops inside cl_unite are bounded as written there.  No workgroup waits
// on another: a workgroup that runs alone finishes
__global__ void __launch_bounds__(kClBlock) cl_union_kernel(const RorPt* __restrict__ pts, const unsigned long long* __restrict__ keys, int n, float r2,
                                                            const int* __restrict__ core, int* parent)
{
	__shared__ RorPt tile[kClBlock];
	__shared__ int tile_core[kClBlock];
	__shared__ int iv_lo[9], iv_hi[9];
	const int tid = threadIdx.x;
	const int first = blockIdx.x * kClBlock, last = min(first + kClBlock, n) - 1;
	const int s = first + tid;
	RorPt P{0.f, 0.f, 0.f, -1};
	long long K = 0;
	bool mine = false;
	if (s < n) { P = pts[s]; K = (long long)keys[s]; mine = core[P.id] != 0; }
	if (!__syncthreads_or(mine)) return;                         // no core point in the span
	grid_intervals(keys, n, first, last, iv_lo, iv_hi);
	for (int o = 0; o < 9; o++) {
		const int lo = iv_lo[o], hi = iv_hi[o];
		for (int t0 = lo; t0 < hi; t0 += kClBlock) {
			__syncthreads();                                     // the previous tile has been read by everybody
			const int len = min(kClBlock, hi - t0);
			if (tid < len) {
				const RorPt Q = pts[t0 + tid];
				tile[tid] = Q;
				tile_core[tid] = core[Q.id];
			}
			__syncthreads();
			const bool need = mine && grid_tile_meets(K, (long long)keys[t0], (long long)keys[t0 + len - 1]);
			if (!need) continue;                                 // the next barrier is at the loop's head, which every lane reaches
			for (int j = 0; j < len; j++) {
				const RorPt Q = tile[j];
				if (!tile_core[j] || Q.id >= P.id) continue;
				const float dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
				const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
				if (d2 <= r2) cl_unite(parent, P.id, Q.id);
			}
		}
	}
}

// after the component kernel has finished: root[i] = the root of core point i, -1 for any other point.  The walk moves to a strictly
// smaller index each step (parent[v] < v for a non-root) and nothing is written to parent any more
__global__ void cl_flatten_kernel(const int* __restrict__ parent, const int* __restrict__ core, int n, int* __restrict__ root)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	int x = -1;
	if (core[i]) {
		x = i;
		for (int p = parent[x]; p != x; p = parent[x]) x = p;
	}
	root[i] = x;
}

// The same tile shape for the points that are not core: the smallest key (bits of d2) << 32 | index over the core candidates within r, then
// that neighbour's root.  root[] is read at core indices and written at the others only
__global__ void __launch_bounds__(kClBlock) cl_border_kernel(const RorPt* __restrict__ pts, const unsigned long long* __restrict__ keys, int n, float r2,
                                                             const int* __restrict__ core, int* root)
{
	__shared__ RorPt tile[kClBlock];
	__shared__ int tile_core[kClBlock];
	__shared__ int iv_lo[9], iv_hi[9];
	const int tid = threadIdx.x;
	const int first = blockIdx.x * kClBlock, last = min(first + kClBlock, n) - 1;
	const int s = first + tid;
	RorPt P{0.f, 0.f, 0.f, -1};
	long long K = 0;
	bool mine = false;
	if (s < n) { P = pts[s]; K = (long long)keys[s]; mine = core[P.id] == 0; }
	if (!__syncthreads_or(mine)) return;                         // every point of the span is core
	grid_intervals(keys, n, first, last, iv_lo, iv_hi);
	unsigned long long best = ~0ull;
	for (int o = 0; o < 9; o++) {
		const int lo = iv_lo[o], hi = iv_hi[o];
		for (int t0 = lo; t0 < hi; t0 += kClBlock) {
			__syncthreads();                                     // the previous tile has been read by everybody
			const int len = min(kClBlock, hi - t0);
			if (tid < len) {
				const RorPt Q = pts[t0 + tid];
				tile[tid] = Q;
				tile_core[tid] = core[Q.id];
			}
			__syncthreads();
			const bool need = mine && grid_tile_meets(K, (long long)keys[t0], (long long)keys[t0 + len - 1]);
			if (!need) continue;                                 // the next barrier is at the loop's head, which every lane reaches
			for (int j = 0; j < len; j++) {
				const RorPt Q = tile[j];
				if (!tile_core[j]) continue;                      // a core point is not P, which is none
				const float dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
				const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
				const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(unsigned)Q.id;
				if (d2 <= r2 && key < best) best = key;
			}
		}
	}
	if (mine && best != ~0ull) root[P.id] = root[(int)(unsigned)(best & 0xffffffffull)];
}

__global__ void cl_rootflag_kernel(const int* __restrict__ root, int n, int* __restrict__ isroot)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) isroot[i] = root[i] == i ? 1 : 0;
}

// scan: the exclusive scan of the root flags, so scan[r] is the dense label of root r; sizes is zeroed and counts by integer atomicAdd
__global__ void cl_label_kernel(const int* __restrict__ root, const int* __restrict__ scan, int n, int32_t* __restrict__ label, int32_t* __restrict__ sizes)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int r = root[i];
	const int l = r < 0 ? -1 : scan[r];
	label[i] = l;
	if (l >= 0) atomicAdd(sizes + l, 1);
}

__global__ void cl_keepflag_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ keep, int n, int* __restrict__ flag)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int l = label[i];
	flag[i] = (l >= 0 && keep[l]) ? 1 : 0;
}

hipError_t launch_cluster(const float* d_xyz, int n, const VoxelFrame& f, float r2, int min_neighbors, int32_t* d_label, int32_t* d_sizes, int* c_out,
                          hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (n <= 0 || !c_out || !d_label || !d_sizes || min_neighbors < 0) return hipErrorInvalidValue;
	const dim3 blk(256), grd((n + 255) / 256), tgrd((n + kClBlock - 1) / kClBlock), tblk(kClBlock);
	int *core = nullptr, *parent = nullptr, *root = nullptr, *isroot = nullptr, *scan = nullptr;
	void* tmp = nullptr;
	Temps t;
	CellGrid g;
	const size_t N = (size_t)n;
	KD_TRY(g.alloc(t, N, true));
	KD_TRY(t.get(core, N));
	KD_TRY(t.get(parent, N));
	KD_TRY(t.get(root, N));
	KD_TRY(t.get(isroot, N + 1));
	KD_TRY(t.get(scan, N + 1));
	size_t sort_bytes = 0, scan_bytes = 0;
	KD_TRY(grid_sort_bytes(g, N, &f, 1, sort_bytes, stream));
	KD_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, isroot, scan, 0, N + 1, rocprim::plus<int>(), stream));
	KD_TRY(t.get_bytes(tmp, std::max<size_t>(std::max(sort_bytes, scan_bytes), 16)));
	// ev_begin .. ev_end: the kernels and the 4-byte read-back of c; the allocations above and the frees at the end are outside
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	KD_TRY(grid_build(d_xyz, n, f, g, tmp, sort_bytes, stream));
	hipLaunchKernelGGL(cl_init_kernel, grd, blk, 0, stream, parent, core, n, min_neighbors == 0 ? 1 : 0);
	KD_TRY(hipGetLastError());
	if (min_neighbors > 0) {
		// the radius filter's saturating count: core[i] = (count_i == min_neighbors); the counts themselves go to root, which is rewritten below
		hipLaunchKernelGGL(ror_count_kernel, tgrd, tblk, 0, stream, g.pts, g.sorted_keys, n, r2, min_neighbors, root, core);
		KD_TRY(hipGetLastError());
	}
	hipLaunchKernelGGL(cl_union_kernel, tgrd, tblk, 0, stream, g.pts, g.sorted_keys, n, r2, core, parent);
	KD_TRY(hipGetLastError());
	hipLaunchKernelGGL(cl_flatten_kernel, grd, blk, 0, stream, parent, core, n, root);
	KD_TRY(hipGetLastError());
	if (min_neighbors > 0) {
		hipLaunchKernelGGL(cl_border_kernel, tgrd, tblk, 0, stream, g.pts, g.sorted_keys, n, r2, core, root);
		KD_TRY(hipGetLastError());
	}
	hipLaunchKernelGGL(cl_rootflag_kernel, grd, blk, 0, stream, root, n, isroot);
	KD_TRY(hipGetLastError());
	KD_TRY(hipMemsetAsync(isroot + N, 0, sizeof(int), stream));
	KD_TRY(rocprim::exclusive_scan(tmp, scan_bytes, isroot, scan, 0, N + 1, rocprim::plus<int>(), stream));
	KD_TRY(hipMemsetAsync(d_sizes, 0, sizeof(int32_t) * N, stream));
	hipLaunchKernelGGL(cl_label_kernel, grd, blk, 0, stream, root, scan, n, d_label, d_sizes);
	KD_TRY(hipGetLastError());
	int c = -1;
	KD_TRY(hipMemcpyAsync(&c, scan + N, sizeof(int), hipMemcpyDeviceToHost, stream));
	KD_TRY(end_and_drain(ev_end, stream));
	if (c < 0 || c > n) return hipErrorUnknown;
	*c_out = c;
	return hipSuccess;
}

hipError_t launch_cluster_compact(const float* d_xyz, int n, const int32_t* d_label, const int32_t* d_keep, float* d_out, int32_t* d_index,
                                  int32_t* d_out_label, int* m_out, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (n <= 0 || !m_out || !d_label || !d_keep || !d_out) return hipErrorInvalidValue;
	int *flag = nullptr, *scan = nullptr;
	void* tmp = nullptr;
	Temps t;
	const size_t N = (size_t)n;
	KD_TRY(t.get(flag, N + 1));
	KD_TRY(t.get(scan, N + 1));
	size_t scan_bytes = 0;
	KD_TRY(compact_scan_bytes(flag, scan, N, scan_bytes, stream));
	KD_TRY(t.get_bytes(tmp, std::max<size_t>(scan_bytes, 16)));
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	hipLaunchKernelGGL(cl_keepflag_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_label, d_keep, n, flag);
	KD_TRY(hipGetLastError());
	int m = -1;
	KD_TRY(compact_tail(d_xyz, n, flag, scan, tmp, scan_bytes, d_label, d_out, d_index, d_out_label, &m, stream));
	KD_TRY(end_and_drain(ev_end, stream));
	if (m < 0 || m > n) return hipErrorUnknown;
	*m_out = m;
	return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// Statistical outlier removal on the device (host twin: statistical_outlier_removal_host, kdtree.cpp).  The k smallest d2 of every
// point are found on grids of doubling radius r_L = r0 2^L (pitch 1.03125 r_L, the radius filter's grid and its proof): a point whose k-th
// smallest d2 over its 27 cells is <= r_L * r_L has seen every point that close, so those k are its k smallest of the whole
// cloud; the others go to a compacted list for the next level, and what the last level leaves scans all points.  Level 0 serves every point
// (grid_knn_block_kernel, the count kernel's shape), the later levels few scattered ones (grid_knn_wave_kernel, a wave per point).  The
// number of levels is fixed by the host; the length of the list comes back between levels (4 bytes) so that an empty one ends the chain.
// The statistics stay on the device: the maximum over float bits, exact 64-bit integer sums, one thread that finishes in fp64.
// ------------------------------------------------------------------------------------------------
constexpr int kStatBlock = 256;

__device__ __forceinline__ float stat_d2(float px, float py, float pz, const RorPt& Q)
{
	const float dx = px - Q.x, dy = py - Q.y, dz = pz - Q.z;
	return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// the correctly rounded float square root: sqrtf, which the build keeps IEEE (the compiler's default for HIP; so_gather_kernel's |p| relies
// on the same).  __fsqrt_rn is the hardware's approximate instruction in this toolchain and differs from the host in the last bit
__device__ __forceinline__ float stat_sqrt(float v) { return sqrtf(v); }

// The search kernels serve this filter and the self k-NN (below), which differ in the entry of the k-best lists and in what a resolved
// point writes.  An entry policy E: the type T, none() (above every candidate), make(d2, id), d2(e) -- of none() a value that is <= no
// radius, so a list with fewer than k entries is never resolved -- and the wave's shuffles.  A sink names its entry policy; lane() is
// called by a resolved lane of the block kernel with its column of the lists (entry j at col[j * kStatBlock]), wave() by every lane of a
// resolved wave (lane j holds entry j)
struct KnnDist {                                               // d2 alone; none = INFINITY
	using T = float;
	static __device__ __forceinline__ T none() { return INFINITY; }
	static __device__ __forceinline__ T make(float d2, int) { return d2; }
	static __device__ __forceinline__ float d2(T e) { return e; }
	static __device__ __forceinline__ T shfl(T e, int src) { return __shfl(e, src, 64); }
	static __device__ __forceinline__ T shfl_up(T e) { return __shfl_up(e, 1, 64); }
};

// u = the mean of the k distances, summed ascending in fp64
struct MeanSink {
	using Entry = KnnDist;
	float* __restrict__ u;
	__device__ __forceinline__ void lane(int id, int k, const float* col) const
	{
		double sum = 0.0;
		for (int j = 0; j < k; j++) sum = __dadd_rn(sum, (double)stat_sqrt(col[j * kStatBlock]));
		u[id] = (float)__ddiv_rn(sum, (double)k);
	}
	__device__ __forceinline__ void wave(int id, int k, int lane, float mine) const
	{
		double sum = 0.0;
		for (int j = 0; j < k; j++) sum = __dadd_rn(sum, (double)stat_sqrt(__shfl(mine, j, 64)));
		if (lane == 0) u[id] = (float)__ddiv_rn(sum, (double)k);
	}
};

// The count kernel's shape: a workgroup owns kStatBlock consecutive SORTED points and passes the candidate intervals of its span
// (grid_intervals) through LDS in tiles; a wave skips a tile that meets none of its lanes' runs, and a lane takes only tiles that meet its
// own.  Each lane keeps its k smallest entries ascending in LDS at stride kStatBlock (lane t owns column t: no two lanes of a wave share a
// bank column; of 8-byte entries the 32 lanes of a half wave read 64 consecutive dwords, one bank each), KT >= k rows of 1 or 2 KB.  A
// candidate is inserted only when strictly below the lane's k-th entry, held in registers, so ties of d2 and a cell of identical points
// cost nothing; keys are unique, so there a cell of identical points costs one comparison per candidate once the column holds the k
// smallest indices.  A lane whose k-th d2 is <= r2 hands its column to the sink; any other appends its id to the open list.  No workgroup
// waits on another
template <int KT, class Sink>
__global__ void __launch_bounds__(kStatBlock) grid_knn_block_kernel(const RorPt* __restrict__ pts, const unsigned long long* __restrict__ keys, int n, int k,
                                                                    float r2, Sink sink, int* __restrict__ open_list, int* __restrict__ open_count)
{
	using E = typename Sink::Entry;
	using T = typename E::T;
	__shared__ RorPt tile[kStatBlock];
	__shared__ T best[KT * kStatBlock];
	__shared__ int iv_lo[9], iv_hi[9];
	const int tid = threadIdx.x;
	const int first = blockIdx.x * kStatBlock, last = min(first + kStatBlock, n) - 1;
	const int s = first + tid;
	const bool valid = s < n;
	for (int j = 0; j < k; j++) best[j * kStatBlock + tid] = E::none();
	grid_intervals(keys, n, first, last, iv_lo, iv_hi);
	RorPt P{0.f, 0.f, 0.f, -1};
	long long K = 0;
	if (valid) { P = pts[s]; K = (long long)keys[s]; }
	T kth = E::none();
	for (int o = 0; o < 9; o++) {
		const int lo = iv_lo[o], hi = iv_hi[o];
		for (int t0 = lo; t0 < hi; t0 += kStatBlock) {
			__syncthreads();                                     // the previous tile has been read by everybody
			const int len = min(kStatBlock, hi - t0);
			if (tid < len) tile[tid] = pts[t0 + tid];
			__syncthreads();
			const bool need = valid && grid_tile_meets(K, (long long)keys[t0], (long long)keys[t0 + len - 1]);
			if (!__any(need)) continue;                          // wave-uniform; the next barrier is at the loop's head
			if (!need) continue;
			for (int j = 0; j < len; j++) {
				const RorPt Q = tile[j];
				const T c = E::make(stat_d2(P.x, P.y, P.z, Q), Q.id);
				if (c < kth && Q.id != P.id) {
					int p = k - 1;
					while (p > 0) {
						const T b = best[(p - 1) * kStatBlock + tid];
						if (!(b > c)) break;
						best[p * kStatBlock + tid] = b;
						p--;
					}
					best[p * kStatBlock + tid] = c;
					kth = best[(k - 1) * kStatBlock + tid];
				}
			}
		}
	}
	if (!valid) return;
	if (E::d2(kth) <= r2) sink.lane(P.id, k, best + tid);
	else open_list[atomicAdd(open_count, 1)] = P.id;
}

// A wave per listed point.  Lanes 0..8 find the point's own 9 runs [K + D - 1, K + D + 1] (disjoint key ranges: no candidate is offered
// twice); all = 1 is the top level, the one run [0, n).  The lanes read 64 candidates at a time; lane j holds the j-th smallest entry seen
// so far in registers, and a candidate v strictly below the k-th entry is inserted by one shuffle up: a lane keeps its entry if it is
// <= v, takes v if its lower neighbour's entry is <= v, and its lower neighbour's entry otherwise.  (Keys are unique, every candidate is
// offered once and v is never none(), so of keys no entry equals v and <= reads as <.)  The loops run over the runs' lengths, which the
// host's number of levels bounds; no wave waits on another
template <class Sink>
__global__ void __launch_bounds__(256) grid_knn_wave_kernel(const float* __restrict__ xyz, const RorPt* __restrict__ pts, const unsigned long long* __restrict__ keys,
                                                            int n, const int* __restrict__ list, int count, int k, float r2, int all, float mnx, float mny,
                                                            float mnz, float pitch, Sink sink, int* __restrict__ open_list, int* __restrict__ open_count)
{
	using E = typename Sink::Entry;
	using T = typename E::T;
	const int w = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
	if (w >= count) return;                                      // wave-uniform
	const int id = list[w];
	const float px = xyz[3 * (size_t)id], py = xyz[3 * (size_t)id + 1], pz = xyz[3 * (size_t)id + 2];
	int my_lo = 0, my_hi = 0;
	if (all) {
		if (lane == 0) my_hi = n;
	} else if (lane < 9) {
		const long long K = (long long)(vx_cell(px - mnx, pitch) | (vx_cell(py - mny, pitch) << 21) | (vx_cell(pz - mnz, pitch) << 42));
		const long long c = K + (long long)(lane % 3 - 1) * (1ll << 21) + (long long)(lane / 3 - 1) * (1ll << 42);
		my_lo = ror_bound(keys, n, c - 1, false);
		my_hi = max(my_lo, ror_bound(keys, n, c + 1, true));
	}
	T mine = E::none(), kth = E::none();
	const int runs = all ? 1 : 9;
	for (int o = 0; o < runs; o++) {
		const int lo = __shfl(my_lo, o, 64), hi = __shfl(my_hi, o, 64);
		for (int base = lo; base < hi; base += 64) {
			const int j = base + lane;
			T c = E::none();
			if (j < hi) {
				const RorPt Q = pts[j];
				if (Q.id != id) c = E::make(stat_d2(px, py, pz, Q), Q.id);
			}
			unsigned long long hot = __ballot(c < kth);
			while (hot) {
				const int src = __ffsll((long long)hot) - 1;
				hot &= hot - 1;
				const T v = E::shfl(c, src);
				if (v < kth) {                                       // wave-uniform
					const T below = E::shfl_up(mine);
					mine = (mine <= v) ? mine : ((lane == 0 || below <= v) ? v : below);
					kth = E::shfl(mine, k - 1);
				}
			}
		}
	}
	if (all || E::d2(kth) <= r2) sink.wave(id, k, lane, mine);
	else if (lane == 0) open_list[atomicAdd(open_count, 1)] = id;
}

// what the finishing thread leaves for the flags and the host
struct StatFinish { double Tq, threshold; int e, all; };

// U over the bits of u: non-negative floats order as unsigned integers
__global__ void __launch_bounds__(256) stat_max_kernel(const float* __restrict__ u, int n, unsigned* __restrict__ umax)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned b = i < n ? __float_as_uint(u[i]) : 0u;
	for (int off = 32; off; off >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, off, 64));
	if ((threadIdx.x & 63) == 0 && b) atomicMax(umax, b);
}

__device__ __forceinline__ unsigned long long stat_q(float u, int e) { return (unsigned long long)(long long)floor(ldexp((double)u, 31 - e)); }

// sums[0..2] = S1, A, B: exact integers, so the order in which the waves arrive cannot matter
__global__ void __launch_bounds__(256) stat_sums_kernel(const float* __restrict__ u, int n, const unsigned* __restrict__ umax, unsigned long long* __restrict__ sums)
{
	const unsigned ub = *umax;
	if (!ub) return;
	int e = 0;
	frexpf(__uint_as_float(ub), &e);
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned long long q = i < n ? stat_q(u[i], e) : 0ull;
	unsigned long long s1 = q, a = (q * q) >> 32, b = (q * q) & 0xffffffffull;
	for (int off = 32; off; off >>= 1) { s1 += shfl_xor64(s1, off); a += shfl_xor64(a, off); b += shfl_xor64(b, off); }
	if ((threadIdx.x & 63) == 0) { atomicAdd(sums, s1); atomicAdd(sums + 1, a); atomicAdd(sums + 2, b); }
}

// one thread: the finish of the header in fp64, each operation rounded once
__global__ void stat_finish_kernel(const unsigned* __restrict__ umax, const unsigned long long* __restrict__ sums, int n, float alpha, StatFinish* __restrict__ fin)
{
	if (blockIdx.x || threadIdx.x) return;
	StatFinish r{0.0, 0.0, 0, 1};
	const unsigned ub = *umax;
	if (ub) {
		frexpf(__uint_as_float(ub), &r.e);
		const double S1 = (double)(long long)sums[0], A = (double)(long long)sums[1], B = (double)(long long)sums[2];
		const double nd = (double)n;
		const double mean = __ddiv_rn(S1, nd);
		const double S2 = __dadd_rn(ldexp(A, 32), B);
		double var = __ddiv_rn(__dsub_rn(S2, __dmul_rn(S1, mean)), __dsub_rn(nd, 1.0));
		if (!(var > 0.0)) var = 0.0;
		r.Tq = __dadd_rn(mean, __dmul_rn((double)alpha, __dsqrt_rn(var)));
		r.threshold = ldexp(r.Tq, r.e - 31);
		r.all = 0;
	}
	*fin = r;
}

__global__ void stat_flag_kernel(const float* __restrict__ u, int n, const StatFinish* __restrict__ fin, int* __restrict__ flag)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	flag[i] = (fin->all || (double)(long long)stat_q(u[i], fin->e) <= fin->Tq) ? 1 : 0;
}

// The levels of a search, for both of its users.  Level 0 serves every point -- block(r2, open_list, open_count) launches the caller's
// block kernel -- and every later level the listed ones: wave(list, count, r2, all, frame, open_list, open_count) launches its wave
// kernel.  After each level the length of the open list comes back (4 bytes), so that an empty one ends the chain, and the lists swap;
// what the last level leaves goes to the top level, where every point is a candidate, in any order (all = 1: the frame is not read).
// g.order and g.pts start as level 0's or, with no level, as the input order, which the top level's records and list then need; that
// first order is what d_order (may be null) receives.  n >= 2 points are open before level 0, so a search with levels runs level 0.
// cur / nxt: n ints each; counts: kStatMaxLevels + 1 zeroed ints, one per level and the top level's
template <class Block, class Wave>
static hipError_t grid_knn_levels(const float* d_xyz, int n, const VoxelFrame* frames, const float* r2, int levels, const CellGrid& g, void* tmp,
                                  size_t sort_bytes, int* cur, int* nxt, int* counts, int* d_order, StatReport& rep, hipStream_t stream, Block block,
                                  Wave wave)
{
	const dim3 blk(256), grd((n + 255) / 256);
	if (levels > 0) {
		KD_TRY(grid_build(d_xyz, n, frames[0], g, tmp, sort_bytes, stream));
	} else {
		hipLaunchKernelGGL(so_iota_kernel, grd, blk, 0, stream, g.order, n);
		KD_TRY(hipGetLastError());
		hipLaunchKernelGGL(so_iota_kernel, grd, blk, 0, stream, cur, n);
		KD_TRY(hipGetLastError());
		hipLaunchKernelGGL(ror_gather_kernel, grd, blk, 0, stream, d_xyz, g.order, n, g.pts);
		KD_TRY(hipGetLastError());
	}
	if (d_order) KD_TRY(hipMemcpyAsync(d_order, g.order, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, stream));
	int open = n;                                              // the points no level has resolved yet
	for (int L = 0; L < levels && open > 0; L++) {
		if (L == 0) {
			block(r2[0], nxt, counts);
		} else {
			KD_TRY(grid_build(d_xyz, n, frames[L], g, tmp, sort_bytes, stream));
			wave(cur, open, r2[L], 0, frames[L], nxt, counts + L);
		}
		KD_TRY(hipGetLastError());
		int left = -1;
		KD_TRY(hipMemcpyAsync(&left, counts + L, sizeof(int), hipMemcpyDeviceToHost, stream));
		KD_TRY(hipStreamSynchronize(stream));
		if (left < 0 || left > open) return hipErrorUnknown;
		rep.resolved[L] = open - left;
		rep.levels_run = L + 1;
		open = left;
		std::swap(cur, nxt);
	}
	if (open > 0) {
		const VoxelFrame unread{{0.f, 0.f, 0.f}, 0.f, 1.f, 0, 0};
		wave(cur, open, 0.f, 1, unread, nxt, counts + kStatMaxLevels);
		KD_TRY(hipGetLastError());
		rep.top = open;
	}
	return hipSuccess;
}

static dim3 knn_wave_grid(int count) { return dim3((unsigned)(((size_t)count * 64 + 255) / 256)); }

hipError_t launch_stat_outlier_removal(const float* d_xyz, int n, const VoxelFrame* frames, const float* r2, int levels, int k, float std_ratio,
                                       float* d_out, int32_t* d_index, float* d_mean, double* threshold, int* m_out, StatReport* report, hipStream_t stream,
                                       hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (n < 2 || !m_out || k < 1 || k > 64 || k > n - 1 || levels < 0 || levels > kStatMaxLevels || (levels > 0 && (!frames || !r2))) return hipErrorInvalidValue;
	const dim3 blk(256), grd((n + 255) / 256);
	unsigned long long* sums = nullptr;
	int *flag = nullptr, *scan = nullptr, *listA = nullptr, *listB = nullptr, *counts = nullptr;
	float* mean = nullptr;
	StatFinish* fin = nullptr;
	void* tmp = nullptr;
	Temps t;
	CellGrid g;
	const size_t N = (size_t)n;
	KD_TRY(g.alloc(t, N, true));
	KD_TRY(t.get(sums, 4));                                      // S1, A, B and the bits of U
	KD_TRY(t.get(flag, N + 1));
	KD_TRY(t.get(scan, N + 1));
	KD_TRY(t.get(listA, N));
	KD_TRY(t.get(listB, N));
	KD_TRY(t.get(counts, kStatMaxLevels + 1));
	KD_TRY(t.get(fin, 1));
	if (!d_mean) KD_TRY(t.get(mean, N));
	float* u = d_mean ? d_mean : mean;
	unsigned* umax = (unsigned*)(sums + 3);
	size_t sort_bytes = 0, scan_bytes = 0;
	KD_TRY(grid_sort_bytes(g, N, frames, levels, sort_bytes, stream));
	KD_TRY(compact_scan_bytes(flag, scan, N, scan_bytes, stream));
	KD_TRY(t.get_bytes(tmp, std::max<size_t>(std::max(sort_bytes, scan_bytes), 16)));
	StatReport rep;
	// ev_begin .. ev_end: the kernels and the read-backs; the allocations above and the frees at the end are outside
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	KD_TRY(hipMemsetAsync(counts, 0, sizeof(int) * (kStatMaxLevels + 1), stream));
	KD_TRY(hipMemsetAsync(sums, 0, sizeof(unsigned long long) * 4, stream));
	const MeanSink sink{u};
	KD_TRY(grid_knn_levels(
		d_xyz, n, frames, r2, levels, g, tmp, sort_bytes, listA, listB, counts, nullptr, rep, stream,
		[&](float r2_0, int* open_list, int* open_count) {
			const dim3 g0((n + kStatBlock - 1) / kStatBlock), b0(kStatBlock);
			if (k <= 16) hipLaunchKernelGGL((grid_knn_block_kernel<16, MeanSink>), g0, b0, 0, stream, g.pts, g.sorted_keys, n, k, r2_0, sink, open_list, open_count);
			else if (k <= 32) hipLaunchKernelGGL((grid_knn_block_kernel<32, MeanSink>), g0, b0, 0, stream, g.pts, g.sorted_keys, n, k, r2_0, sink, open_list, open_count);
			else hipLaunchKernelGGL((grid_knn_block_kernel<64, MeanSink>), g0, b0, 0, stream, g.pts, g.sorted_keys, n, k, r2_0, sink, open_list, open_count);
		},
		[&](const int* list, int count, float r2_L, int all, const VoxelFrame& f, int* open_list, int* open_count) {
			hipLaunchKernelGGL(grid_knn_wave_kernel<MeanSink>, knn_wave_grid(count), blk, 0, stream, d_xyz, g.pts, g.sorted_keys, n, list, count, k, r2_L, all,
			                   f.mn[0], f.mn[1], f.mn[2], f.voxel, sink, open_list, open_count);
		}));
	hipLaunchKernelGGL(stat_max_kernel, grd, blk, 0, stream, u, n, umax);
	KD_TRY(hipGetLastError());
	hipLaunchKernelGGL(stat_sums_kernel, grd, blk, 0, stream, u, n, umax, sums);
	KD_TRY(hipGetLastError());
	hipLaunchKernelGGL(stat_finish_kernel, dim3(1), dim3(64), 0, stream, umax, sums, n, std_ratio, fin);
	KD_TRY(hipGetLastError());
	hipLaunchKernelGGL(stat_flag_kernel, grd, blk, 0, stream, u, n, fin, flag);
	KD_TRY(hipGetLastError());
	int m = -1;
	StatFinish h_fin{0.0, 0.0, 0, 0};
	KD_TRY(compact_tail(d_xyz, n, flag, scan, tmp, scan_bytes, nullptr, d_out, d_index, nullptr, &m, stream));
	KD_TRY(hipMemcpyAsync(&h_fin, fin, sizeof(StatFinish), hipMemcpyDeviceToHost, stream));
	KD_TRY(end_and_drain(ev_end, stream));
	if (m < 1 || m > n) return hipErrorUnknown;
	*m_out = m;
	if (threshold) *threshold = h_fin.threshold;
	if (report) *report = rep;
	return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// Exact self k-NN and normal estimation on the device (host twins: knn_self_host, estimate_normals_host, kdtree.cpp).  The
// statistical filter's search with the neighbours kept, not only their distances: every candidate is the 64-bit key
// (bits of d2) << 32 | index, a total order, so the k smallest keys are the rows the header defines, ties at the k-th place included.  A
// point is resolved at level L when the d2 of its k-th key is <= r_L * r_L: every point that close lies in its 27 cells, so
// no unseen point has a smaller key.  Level 0 serves every point (grid_knn_block_kernel with keys), the later levels and the top level the
// listed ones (grid_knn_wave_kernel with keys); normal_pca_kernel turns the rows into normals, one thread per point.
// ------------------------------------------------------------------------------------------------
constexpr unsigned long long kKnnNoKey = ~0ull;                // above every key: the d2 of a key is finite

struct KnnKey {                                                // (bits of d2) << 32 | index; none = kKnnNoKey
	using T = unsigned long long;
	static __device__ __forceinline__ T none() { return kKnnNoKey; }
	static __device__ __forceinline__ T make(float d2, int id) { return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(unsigned)id; }
	// the d2 of a key; of kKnnNoKey a NaN, which is <= no radius
	static __device__ __forceinline__ float d2(T key) { return __uint_as_float((unsigned)(key >> 32)); }
	static __device__ __forceinline__ T shfl(T key, int src) { return shfl64(key, src); }
	static __device__ __forceinline__ T shfl_up(T key) { return shfl_up64(key, 1); }
};

// row id of the index matrix and, when asked for, of the d2 matrix
struct RowSink {
	using Entry = KnnKey;
	int32_t* __restrict__ index;
	float* __restrict__ d2;
	__device__ __forceinline__ void put(size_t at, unsigned long long key) const
	{
		index[at] = (int32_t)(unsigned)(key & 0xffffffffull);
		if (d2) d2[at] = KnnKey::d2(key);
	}
	__device__ __forceinline__ void lane(int id, int k, const unsigned long long* col) const
	{
		const size_t row = (size_t)id * (size_t)k;
		for (int j = 0; j < k; j++) put(row + j, col[j * kStatBlock]);
	}
	__device__ __forceinline__ void wave(int id, int k, int lane, unsigned long long mine) const
	{
		if (lane < k) put((size_t)id * (size_t)k + (size_t)lane, mine);
	}
};

// One thread per point, taken in the order of the first grid level so that the threads of a wave gather from neighbouring memory.  The
// arithmetic is normal_pca_point's (device.hpp), the host's text
__global__ void __launch_bounds__(256) normal_pca_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ rows, const int* __restrict__ order, int n,
                                                         int kk, int has_vp, float vpx, float vpy, float vpz, float* __restrict__ normals,
                                                         float* __restrict__ variation)
{
	const int s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const int i = order[s];
	float nrm[3], var;
	normal_pca_point(xyz, i, rows + (size_t)i * (size_t)kk, kk, has_vp != 0, vpx, vpy, vpz, nrm, &var);
	normals[3 * (size_t)i] = nrm[0]; normals[3 * (size_t)i + 1] = nrm[1]; normals[3 * (size_t)i + 2] = nrm[2];
	if (variation) variation[i] = var;
}

hipError_t launch_self_knn(const float* d_xyz, int n, const VoxelFrame* frames, const float* r2, int levels, int k, int32_t* d_index, float* d_dist_sq,
                           int* d_order, StatReport* report, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (n < 2 || !d_index || k < 1 || k > kKnnSelfMax || k > n - 1 || levels < 0 || levels > kStatMaxLevels || (levels > 0 && (!frames || !r2))) return hipErrorInvalidValue;
	int *listA = nullptr, *listB = nullptr, *counts = nullptr;
	void* tmp = nullptr;
	Temps t;
	CellGrid g;
	const size_t N = (size_t)n;
	KD_TRY(g.alloc(t, N, true));
	KD_TRY(t.get(listA, N));
	KD_TRY(t.get(listB, N));
	KD_TRY(t.get(counts, kStatMaxLevels + 1));
	size_t sort_bytes = 0;
	KD_TRY(grid_sort_bytes(g, N, frames, levels, sort_bytes, stream));
	KD_TRY(t.get_bytes(tmp, std::max<size_t>(sort_bytes, 16)));
	StatReport rep;
	// ev_begin .. ev_end: the kernels and the read-backs; the allocations above and the frees at the end are outside
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	KD_TRY(hipMemsetAsync(counts, 0, sizeof(int) * (kStatMaxLevels + 1), stream));
	const RowSink sink{d_index, d_dist_sq};
	KD_TRY(grid_knn_levels(
		d_xyz, n, frames, r2, levels, g, tmp, sort_bytes, listA, listB, counts, d_order, rep, stream,
		[&](float r2_0, int* open_list, int* open_count) {
			const dim3 g0((n + kStatBlock - 1) / kStatBlock), b0(kStatBlock);
			if (k <= 16) hipLaunchKernelGGL((grid_knn_block_kernel<16, RowSink>), g0, b0, 0, stream, g.pts, g.sorted_keys, n, k, r2_0, sink, open_list, open_count);
			else hipLaunchKernelGGL((grid_knn_block_kernel<32, RowSink>), g0, b0, 0, stream, g.pts, g.sorted_keys, n, k, r2_0, sink, open_list, open_count);
		},
		[&](const int* list, int count, float r2_L, int all, const VoxelFrame& f, int* open_list, int* open_count) {
			hipLaunchKernelGGL(grid_knn_wave_kernel<RowSink>, knn_wave_grid(count), dim3(256), 0, stream, d_xyz, g.pts, g.sorted_keys, n, list, count, k, r2_L, all,
			                   f.mn[0], f.mn[1], f.mn[2], f.voxel, sink, open_list, open_count);
		}));
	KD_TRY(end_and_drain(ev_end, stream));
	if (report) *report = rep;
	return hipSuccess;
}

hipError_t launch_estimate_normals(const float* d_xyz, int n, const VoxelFrame* frames, const float* r2, int levels, int k, const float* vp,
                                   float* d_normals, float* d_variation, int32_t* d_index, StatReport* report, hipStream_t stream, hipEvent_t ev_begin,
                                   hipEvent_t ev_end)
{
	if (n < 3 || !d_normals || !d_index || k < 3 || k > kKnnSelfMax || k - 1 > n - 1) return hipErrorInvalidValue;
	int* order = nullptr;
	Temps t;
	KD_TRY(t.get(order, (size_t)n));
	// ev_begin is recorded by the search, ev_end after the PCA
	KD_TRY(launch_self_knn(d_xyz, n, frames, r2, levels, k - 1, d_index, nullptr, order, report, stream, ev_begin, nullptr));
	hipLaunchKernelGGL(normal_pca_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_xyz, d_index, order, n, k - 1, vp ? 1 : 0, vp ? vp[0] : 0.f,
	                   vp ? vp[1] : 0.f, vp ? vp[2] : 0.f, d_normals, d_variation);
	KD_TRY(hipGetLastError());
	return end_and_drain(ev_end, stream);                      // `order` is in use until here
}

// ------------------------------------------------------------------------------------------------
// FPFH descriptors and descriptor matching on the device (host twins: fpfh_host, match_features_host, kdtree.cpp).  The self
// k-NN's rows stay on the device; spfh_kernel counts the pair features of every point with its row, fpfh_kernel adds the neighbours'
// counts in row order.  Neither kernel parallelises over the neighbours: the order of addition is part of the definition.
// ------------------------------------------------------------------------------------------------
constexpr int kSpfhBlock = 256;
constexpr int kFpfhPoints = 15, kFpfhBlock = 512;              // 15 points x 33 bins = 495 of a workgroup's 512 lanes
static_assert(kFpfhPoints * kFpfhDim <= kFpfhBlock && kKnnSelfMax <= kFpfhDim, "fpfh_kernel: one lane per (point, bin), and per (point, neighbour)");

// One thread per point, in the order of the first grid level as normal_pca_kernel takes them.  The 33 counters of a lane are a byte column
// of LDS (a count is at most k <= 32): indexed by a computed bin they would otherwise live in scratch.  The arithmetic is
// fpfh::pair_bins' (device.hpp), the host's text
__global__ void __launch_bounds__(kSpfhBlock) spfh_kernel(const float* __restrict__ xyz, const float* __restrict__ nrm, const int32_t* __restrict__ rows,
                                                          const int* __restrict__ order, int n, int k, unsigned char* __restrict__ counts)
{
	__shared__ unsigned char cnt[kFpfhDim * kSpfhBlock];
	const int tid = threadIdx.x, s = blockIdx.x * kSpfhBlock + tid;
	if (s >= n) return;                                          // no barrier below: a lane touches its own column alone
	for (int b = 0; b < kFpfhDim; b++) cnt[b * kSpfhBlock + tid] = 0;
	const int i = order[s];
	const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
	const float m[3] = {nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2]};
	const int32_t* row = rows + (size_t)i * (size_t)k;
	for (int j = 0; j < k; j++) {
		const size_t q = (size_t)row[j];
		const float pq[3] = {xyz[3 * q], xyz[3 * q + 1], xyz[3 * q + 2]};
		const float mq[3] = {nrm[3 * q], nrm[3 * q + 1], nrm[3 * q + 2]};
		int b[3];
		if (!fpfh::pair_bins(p, m, pq, mq, b)) continue;
		cnt[b[0] * kSpfhBlock + tid]++;
		cnt[(kFpfhBins + b[1]) * kSpfhBlock + tid]++;
		cnt[(2 * kFpfhBins + b[2]) * kSpfhBlock + tid]++;
	}
	unsigned char* out = counts + (size_t)i * kFpfhDim;
	for (int b = 0; b < kFpfhDim; b++) out[b] = cnt[b * kSpfhBlock + tid];
}

// One lane per (point, bin), 15 points per workgroup: every lane walks its point's row in key order and adds its bin of the neighbours'
// counts; the weights 1 / d2 and the neighbours' ids are formed once per (point, neighbour) in LDS.  A neighbour at d2 == 0 has weight 0
// here and is skipped as the definition says (no 1 / d2 of a float is 0).  The group sums add the 11 LDS values in bin order in every lane
__global__ void __launch_bounds__(kFpfhBlock) fpfh_kernel(const int32_t* __restrict__ rows, const float* __restrict__ d2, const unsigned char* __restrict__ counts,
                                                          const int* __restrict__ order, int n, int k, float* __restrict__ out)
{
	__shared__ double acc[kFpfhPoints * kFpfhDim];
	__shared__ double weight[kFpfhPoints * kKnnSelfMax];
	__shared__ int32_t nb[kFpfhPoints * kKnnSelfMax];
	const int tid = threadIdx.x, p = tid / kFpfhDim, b = tid - p * kFpfhDim;
	const int s = blockIdx.x * kFpfhPoints + p;
	const bool live = p < kFpfhPoints && s < n;
	const int i = live ? order[s] : 0;
	if (live && b < k) {
		const size_t at = (size_t)i * (size_t)k + (size_t)b;
		const float w2 = d2[at];
		weight[p * kKnnSelfMax + b] = w2 == 0.f ? 0.0 : __ddiv_rn(1.0, (double)w2);
		nb[p * kKnnSelfMax + b] = rows[at];
	}
	__syncthreads();
	const double inc = __ddiv_rn(100.0, (double)k);
	double a = 0.0;
	if (live) {
		for (int j = 0; j < k; j++) {
			const double w = weight[p * kKnnSelfMax + j];
			if (!(w > 0.0)) continue;
			const double c = (double)counts[(size_t)nb[p * kKnnSelfMax + j] * kFpfhDim + b];
			a = __dadd_rn(a, __dmul_rn(__dmul_rn(c, inc), w));
		}
		acc[tid] = a;
	}
	__syncthreads();
	if (!live) return;
	const int g = b / kFpfhBins;
	double sum = 0.0;
	for (int c = 0; c < kFpfhBins; c++) sum = __dadd_rn(sum, acc[p * kFpfhDim + g * kFpfhBins + c]);
	if (sum > 0.0) a = __dmul_rn(a, __ddiv_rn(100.0, sum));
	const double own = (double)counts[(size_t)i * kFpfhDim + b];
	out[(size_t)i * kFpfhDim + b] = (float)__dadd_rn(a, __dmul_rn(own, inc));
}

hipError_t launch_fpfh(const float* d_xyz, const float* d_normals, int n, const VoxelFrame* frames, const float* r2, int levels, int k, int32_t* d_index,
                       float* d_dist_sq, unsigned char* d_counts, float* d_fpfh, StatReport* report, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (n < 2 || !d_normals || !d_index || !d_dist_sq || !d_counts || !d_fpfh || k < 1 || k > kKnnSelfMax || k > n - 1) return hipErrorInvalidValue;
	int* order = nullptr;
	Temps t;
	KD_TRY(t.get(order, (size_t)n));
	// ev_begin is recorded by the search, ev_end after the two kernels
	KD_TRY(launch_self_knn(d_xyz, n, frames, r2, levels, k, d_index, d_dist_sq, order, report, stream, ev_begin, nullptr));
	hipLaunchKernelGGL(spfh_kernel, dim3((n + kSpfhBlock - 1) / kSpfhBlock), dim3(kSpfhBlock), 0, stream, d_xyz, d_normals, d_index, order, n, k, d_counts);
	KD_TRY(hipGetLastError());
	hipLaunchKernelGGL(fpfh_kernel, dim3((n + kFpfhPoints - 1) / kFpfhPoints), dim3(kFpfhBlock), 0, stream, d_index, d_dist_sq, d_counts, order, n, k, d_fpfh);
	KD_TRY(hipGetLastError());
	return end_and_drain(ev_end, stream);                      // `order` is in use until here
}

// Brute-force nearest descriptor.  A workgroup of 256 lanes keeps one query per lane in registers and walks a chunk of the targets in
// tiles of kMatchTile descriptors staged in LDS; every lane of a wave reads the same target word at a time (an LDS broadcast), and a row of
// kMatchRow = 36 words keeps the 128-bit reads aligned.  The sum is the definition's: left to right, nothing fused, no matrix instruction.
// blockIdx.y splits the targets into chunks so that few queries still fill the device; partial: [chunk][query][2] keys
constexpr int kMatchBlock = 256;
static_assert(kMatchRow % 4 == 0 && kMatchRow >= kFpfhDim && kFpfhDim == 33, "match_tile_kernel reads a row as eight float4 and one float");

// the two smallest keys seen, by value: x = the smallest, y = the second
__device__ __forceinline__ ulonglong2 match_offer(unsigned long long key, ulonglong2 two)
{
	const bool first = key < two.x, second = key < two.y;
	return make_ulonglong2(first ? key : two.x, first ? two.x : (second ? key : two.y));
}

__global__ void __launch_bounds__(kMatchBlock) match_tile_kernel(const float* __restrict__ q, int nq, const float* __restrict__ t, int nt, int chunk_targets,
                                                                 unsigned long long* __restrict__ partial)
{
	__shared__ float4 tile4[kMatchTile * kMatchRow / 4];
	float* tile = reinterpret_cast<float*>(tile4);
	const int tid = threadIdx.x, qi = blockIdx.x * kMatchBlock + tid;
	const bool live = qi < nq;
	float v[kFpfhDim];
#pragma unroll
	for (int c = 0; c < kFpfhDim; c++) v[c] = live ? q[(size_t)qi * kFpfhDim + c] : 0.f;
	ulonglong2 two = make_ulonglong2(kKnnNoKey, kKnnNoKey);
	const int t0 = blockIdx.y * chunk_targets, t1 = min(nt, t0 + chunk_targets);
	for (int base = t0; base < t1; base += kMatchTile) {
		const int rows = min(kMatchTile, t1 - base);
		__syncthreads();                                         // the previous tile has been read
		for (int e = tid; e < rows * kFpfhDim; e += kMatchBlock) {
			const int r = e / kFpfhDim;
			tile[r * kMatchRow + (e - r * kFpfhDim)] = t[(size_t)base * kFpfhDim + (size_t)e];
		}
		__syncthreads();
		for (int r = 0; r < rows; r++) {
			const float4* row = tile4 + r * (kMatchRow / 4);
			float d2 = 0.f;
#pragma unroll
			for (int w = 0; w < 8; w++) {
				const float4 u = row[w];
				float d = __fsub_rn(v[4 * w], u.x);
				d2 = __fadd_rn(d2, __fmul_rn(d, d));
				d = __fsub_rn(v[4 * w + 1], u.y);
				d2 = __fadd_rn(d2, __fmul_rn(d, d));
				d = __fsub_rn(v[4 * w + 2], u.z);
				d2 = __fadd_rn(d2, __fmul_rn(d, d));
				d = __fsub_rn(v[4 * w + 3], u.w);
				d2 = __fadd_rn(d2, __fmul_rn(d, d));
			}
			const float d = __fsub_rn(v[32], tile[r * kMatchRow + 32]);
			d2 = __fadd_rn(d2, __fmul_rn(d, d));
			two = match_offer(KnnKey::make(d2, base + r), two);
		}
	}
	if (live) {
		const size_t at = ((size_t)blockIdx.y * (size_t)nq + (size_t)qi) * 2;
		partial[at] = two.x;
		partial[at + 1] = two.y;
	}
}

// the two smallest keys of every query over its chunks' pairs (the key order is total, so the merge is exact); d2 / second may be null
__global__ void __launch_bounds__(256) match_merge_kernel(const unsigned long long* __restrict__ partial, int nq, int chunks, int32_t* __restrict__ index,
                                                          float* __restrict__ d2, float* __restrict__ second_d2)
{
	const int qi = blockIdx.x * blockDim.x + threadIdx.x;
	if (qi >= nq) return;
	ulonglong2 two = make_ulonglong2(kKnnNoKey, kKnnNoKey);
	for (int c = 0; c < chunks; c++) {
		const size_t at = ((size_t)c * (size_t)nq + (size_t)qi) * 2;
		two = match_offer(partial[at], two);
		two = match_offer(partial[at + 1], two);             // the "none" key is below no key: it changes nothing
	}
	index[qi] = (int32_t)(unsigned)(two.x & 0xffffffffull);
	if (d2) d2[qi] = KnnKey::d2(two.x);
	if (second_d2) second_d2[qi] = two.y == kKnnNoKey ? __uint_as_float(0x7f800000u) : KnnKey::d2(two.y);
}

// mutual[q] = 1 iff the nearest query of q's nearest target is q
__global__ void __launch_bounds__(256) match_mutual_kernel(const int32_t* __restrict__ index, const int32_t* __restrict__ back, int nq, unsigned char* __restrict__ mutual)
{
	const int qi = blockIdx.x * blockDim.x + threadIdx.x;
	if (qi >= nq) return;
	mutual[qi] = back[index[qi]] == qi ? 1 : 0;
}

// one direction: the smallest key of every one of the nq descriptors of d_q among the nt of d_t, and the d2 of the second smallest
static hipError_t match_direction(const float* d_q, int nq, const float* d_t, int nt, unsigned long long* partial, int chunks, int chunk_targets,
                                  int32_t* d_index, float* d_d2, float* d_second, hipStream_t stream)
{
	hipLaunchKernelGGL(match_tile_kernel, dim3((nq + kMatchBlock - 1) / kMatchBlock, chunks), dim3(kMatchBlock), 0, stream, d_q, nq, d_t, nt, chunk_targets, partial);
	KD_TRY(hipGetLastError());
	hipLaunchKernelGGL(match_merge_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, partial, nq, chunks, d_index, d_d2, d_second);
	return hipGetLastError();
}

// the chunks of nt targets for nq queries: whole tiles, as many chunks as bring the launch to about 2 048 workgroups
static void match_chunks(int nq, int nt, int* chunks, int* chunk_targets)
{
	const int tiles = (nt + kMatchTile - 1) / kMatchTile, qblocks = (nq + kMatchBlock - 1) / kMatchBlock;
	const int want = std::min(tiles, std::max(1, 2048 / qblocks));
	const int per = (tiles + want - 1) / want;
	*chunks = (tiles + per - 1) / per;
	*chunk_targets = per * kMatchTile;
}

hipError_t launch_match_features(const float* d_q, int nq, const float* d_t, int nt, int32_t* d_index, float* d_d2, float* d_second, unsigned char* d_mutual,
                                 hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (nq < 1 || nt < 1 || !d_q || !d_t || !d_index || !d_d2 || !d_second) return hipErrorInvalidValue;
	int chunks = 0, chunk_targets = 0, back_chunks = 0, back_chunk_targets = 0;
	match_chunks(nq, nt, &chunks, &chunk_targets);
	match_chunks(nt, nq, &back_chunks, &back_chunk_targets);
	unsigned long long* partial = nullptr;
	int32_t* back = nullptr;
	Temps tmp;
	size_t words = 2 * (size_t)chunks * (size_t)nq;
	if (d_mutual) words = std::max(words, 2 * (size_t)back_chunks * (size_t)nt);
	KD_TRY(tmp.get(partial, words));
	if (d_mutual) KD_TRY(tmp.get(back, (size_t)nt));
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	KD_TRY(match_direction(d_q, nq, d_t, nt, partial, chunks, chunk_targets, d_index, d_d2, d_second, stream));
	if (d_mutual) {
		// the same stream: the merge above has read `partial` before the transposed call writes it
		KD_TRY(match_direction(d_t, nt, d_q, nq, partial, back_chunks, back_chunk_targets, back, nullptr, nullptr, stream));
		hipLaunchKernelGGL(match_mutual_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, d_index, back, nq, d_mutual);
		KD_TRY(hipGetLastError());
	}
	return end_and_drain(ev_end, stream);                      // the temporaries are in use until here
}

// the per-axis minimum and maximum of a cloud on the device: what voxel_frame derives on the host, for a cloud that never leaves the device
struct MinMax3 { float mn[3], mx[3]; };
struct MinMaxOf {
	const float* xyz;
	__device__ MinMax3 operator()(int i) const
	{
		const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
		return MinMax3{{x, y, z}, {x, y, z}};
	}
};
struct MinMaxJoin {
	__device__ MinMax3 operator()(const MinMax3& a, const MinMax3& b) const
	{
		MinMax3 r;
		for (int k = 0; k < 3; k++) { r.mn[k] = fminf(a.mn[k], b.mn[k]); r.mx[k] = fmaxf(a.mx[k], b.mx[k]); }
		return r;
	}
};

hipError_t launch_cloud_minmax(const float* d_xyz, int n, float mn[3], float mx[3], hipStream_t stream)
{
	if (n <= 0) return hipErrorInvalidValue;
	MinMax3* d_res = nullptr;
	void* tmp = nullptr;
	Temps t;
	auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int>(0), MinMaxOf{d_xyz});
	const MinMax3 init{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
	size_t bytes = 0;
	KD_TRY(rocprim::reduce(nullptr, bytes, in, d_res, init, (size_t)n, MinMaxJoin(), stream));
	KD_TRY(t.get_bytes(tmp, std::max<size_t>(bytes, 16)));
	KD_TRY(t.get(d_res, 1));
	KD_TRY(rocprim::reduce(tmp, bytes, in, d_res, init, (size_t)n, MinMaxJoin(), stream));
	MinMax3 res;
	KD_TRY(hipMemcpyAsync(&res, d_res, sizeof(MinMax3), hipMemcpyDeviceToHost, stream));
	KD_TRY(hipStreamSynchronize(stream));
	for (int k = 0; k < 3; k++) { mn[k] = res.mn[k]; mx[k] = res.mx[k]; }
	return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// RANSAC plane segmentation on the device (host twin: segment_plane_host, kdtree.cpp).  A round is: the hypothesis kernel (one
// thread per hypothesis: the draw and the fp64 plane, device.hpp's text), the score kernel (all points x all hypotheses, integer counts),
// the argmax over (count << 32) | ~t, 8 + 32 bytes to the host; with refine the integer-moment kernel, 128 bytes to the host, plane_refit
// there, the score kernel once more on the one refit plane; then the label kernel and the filters' scan and compaction (compact_tail),
// which form the next round's cloud and carry the index map.
// ------------------------------------------------------------------------------------------------
constexpr int kPlBlock = 256;                                  // threads of a score workgroup: 4 waves
constexpr int kPlPts = 4;                                      // points a lane keeps in registers: 1 024 per workgroup
constexpr int kPlTile = 256;                                   // hypotheses of a workgroup's LDS tile (8 KB of planes + 1 KB of counts)
static_assert(kPlTile == kPlBlock && kPlTile % 64 == 0, "one thread loads one hypothesis of the tile; a wave keeps 64 counts at a time");

// hyp[2 t] = (anchor, 0), hyp[2 t + 1] = (normal, 0) of hypothesis t of the round that starts at number `first`; a degenerate hypothesis gets a
// NaN normal, against which no point is an inlier: it scores 0
__global__ void pl_hyp_kernel(const float* __restrict__ xyz, int n, unsigned long long seed, unsigned long long first, int T, float4* __restrict__ hyp)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= T) return;
	uint32_t a, b, c;
	plane::draw(seed, first + (unsigned long long)t, (uint32_t)n, &a, &b, &c);
	const float pa[3] = {xyz[3 * (size_t)a], xyz[3 * (size_t)a + 1], xyz[3 * (size_t)a + 2]};
	const float pb[3] = {xyz[3 * (size_t)b], xyz[3 * (size_t)b + 1], xyz[3 * (size_t)b + 2]};
	const float pc[3] = {xyz[3 * (size_t)c], xyz[3 * (size_t)c + 1], xyz[3 * (size_t)c + 2]};
	float nr[3];
	const float nan = __int_as_float(0x7fc00000);
	if (!plane::of_triple(pa, pb, pc, nr)) nr[0] = nr[1] = nr[2] = nan;
	hyp[2 * (size_t)t] = make_float4(pa[0], pa[1], pa[2], 0.f);
	hyp[2 * (size_t)t + 1] = make_float4(nr[0], nr[1], nr[2], 0.f);
}

// Workgroup (bx, by): the 1 024 points from bx * 1 024 against the hypotheses by * kPlTile ...  A lane keeps kPlPts points in registers (a
// point past the end is NaN: never an inlier); the tile's planes sit in LDS and are read wave-uniformly; per hypothesis and point the nine
// float operations of the pair, a ballot and a popcount of its 64-bit mask.  The wave's count of hypothesis j0 + jj stays with lane jj, so
// LDS sees one atomic per lane per 64 hypotheses, and global memory one atomic per hypothesis per workgroup
__global__ void __launch_bounds__(kPlBlock) pl_score_kernel(const float* __restrict__ xyz, int n, const float4* __restrict__ hyp, int T, float dist,
                                                            unsigned* __restrict__ counts)
{
	__shared__ float4 s_a[kPlTile], s_n[kPlTile];
	__shared__ unsigned s_cnt[kPlTile];
	const int tid = threadIdx.x, lane = tid & 63;
	const int t0 = blockIdx.y * kPlTile;
	const float nan = __int_as_float(0x7fc00000);
	{
		const int t = t0 + tid;
		s_a[tid] = t < T ? hyp[2 * (size_t)t] : make_float4(0.f, 0.f, 0.f, 0.f);
		s_n[tid] = t < T ? hyp[2 * (size_t)t + 1] : make_float4(nan, nan, nan, 0.f);
		s_cnt[tid] = 0u;
	}
	float px[kPlPts], py[kPlPts], pz[kPlPts];
	const size_t base = (size_t)blockIdx.x * (size_t)(kPlBlock * kPlPts);
#pragma unroll
	for (int k = 0; k < kPlPts; k++) {
		const size_t i = base + (size_t)(k * kPlBlock + tid);
		const bool valid = i < (size_t)n;
		px[k] = valid ? xyz[3 * i] : nan; py[k] = valid ? xyz[3 * i + 1] : nan; pz[k] = valid ? xyz[3 * i + 2] : nan;
	}
	__syncthreads();
	const int live = min(kPlTile, T - t0);                      // the tile's hypotheses that exist; the others have NaN normals
	for (int j0 = 0; j0 < live; j0 += 64) {
		unsigned mine = 0u;
		const int jn = min(64, live - j0);                      // wave-uniform; a lane past it keeps 0 (the refit's re-score has one plane)
		for (int jj = 0; jj < jn; jj++) {
			const float4 a = s_a[j0 + jj], nr = s_n[j0 + jj];
			unsigned c = 0u;
#pragma unroll
			for (int k = 0; k < kPlPts; k++)
				c += (unsigned)__popcll(__ballot(plane::inlier(px[k], py[k], pz[k], a.x, a.y, a.z, nr.x, nr.y, nr.z, dist)));
			mine = lane == jj ? c : mine;
		}
		if (mine) atomicAdd(&s_cnt[j0 + lane], mine);
	}
	__syncthreads();
	if (t0 + tid < T && s_cnt[tid]) atomicAdd(&counts[t0 + tid], s_cnt[tid]);
}

// one workgroup: the largest key (count << 32) | ~t, so the largest count and among equals the smallest t
__global__ void __launch_bounds__(256) pl_argmax_kernel(const unsigned* __restrict__ counts, int T, unsigned long long* __restrict__ best)
{
	__shared__ unsigned long long s_best[4];
	unsigned long long k = 0ull;
	for (int t = threadIdx.x; t < T; t += 256) {
		const unsigned long long key = ((unsigned long long)counts[t] << 32) | (unsigned long long)(~(unsigned)t);
		k = key > k ? key : k;
	}
	for (int off = 32; off; off >>= 1) {
		const unsigned long long o = shfl_xor64(k, off);
		k = o > k ? o : k;
	}
	if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = k;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 4; w++) k = s_best[w] > k ? s_best[w] : k;
		*best = k;
	}
}

// the refit's 16 integer words over the inliers of the plane (a, nr): one thread per point, wave-level sums, then 64-bit atomics (the voxel
// operator's style).  q = llrint(ldexp(x - mn, sh)) < 2^31, so a product has 62 bits and every word of fewer than 2^28 points stays below 2^60
__global__ void __launch_bounds__(256) pl_moment_kernel(const float* __restrict__ xyz, int n, float4 a, float4 nr, float dist, float mnx, float mny, float mnz,
                                                        int sh, unsigned long long* __restrict__ words)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long w[kPlaneWords];
#pragma unroll
	for (int k = 0; k < kPlaneWords; k++) w[k] = 0ull;
	if (i < n) {
		const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
		if (plane::inlier(x, y, z, a.x, a.y, a.z, nr.x, nr.y, nr.z, dist)) {
			const unsigned long long q0 = (unsigned long long)llrint(ldexp((double)(x - mnx), sh)), q1 = (unsigned long long)llrint(ldexp((double)(y - mny), sh)),
			                         q2 = (unsigned long long)llrint(ldexp((double)(z - mnz), sh));
			const unsigned long long p[6] = {q0 * q0, q0 * q1, q0 * q2, q1 * q1, q1 * q2, q2 * q2};
			w[0] = 1ull; w[1] = q0; w[2] = q1; w[3] = q2;
#pragma unroll
			for (int k = 0; k < 6; k++) { w[4 + k] = p[k] >> 32; w[10 + k] = p[k] & 0xffffffffull; }
		}
	}
#pragma unroll
	for (int k = 0; k < kPlaneWords; k++)
		for (int off = 32; off; off >>= 1) w[k] += shfl_xor64(w[k], off);
	if ((threadIdx.x & 63) == 0 && w[0]) {
#pragma unroll
		for (int k = 0; k < kPlaneWords; k++) atomicAdd(words + k, w[k]);
	}
}

// the inliers of the final plane of round `p` get its label (through the index map; null = identity), the others the keep flag
__global__ void pl_label_kernel(const float* __restrict__ xyz, int n, float4 a, float4 nr, float dist, const int* __restrict__ map, int p,
                                int32_t* __restrict__ label, int* __restrict__ flag)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool in = plane::inlier(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], a.x, a.y, a.z, nr.x, nr.y, nr.z, dist);
	if (in && label) label[map ? map[i] : i] = p;
	flag[i] = in ? 0 : 1;
}

hipError_t launch_segment_plane(const float* d_xyz, int n, const PlaneSelect& s, int32_t* d_label, float* d_out, int32_t* d_index, PlaneRecord* planes,
                                int* n_planes, int* m_out, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (n <= 0 || !planes || !n_planes || !m_out || (d_index && !d_out)) return hipErrorInvalidValue;
	if (s.iterations < 1 || s.iterations > kPlaneMaxIterations || s.max_planes < 1 || s.max_planes > kPlaneMaxPlanes) return hipErrorInvalidValue;
	const int T = s.iterations;
	const size_t N = (size_t)n;
	float *buf[2] = {nullptr, nullptr};
	int *mapbuf[2] = {nullptr, nullptr}, *flag = nullptr, *scan = nullptr;
	float4* hyp = nullptr;
	unsigned* counts = nullptr;
	unsigned long long* small = nullptr;                         // [0] the best key, [1..16] the moment words
	void* tmp = nullptr;
	Temps t;
	KD_TRY(t.get(flag, N + 1));
	KD_TRY(t.get(hyp, 2 * (size_t)T));
	KD_TRY(t.get(counts, (size_t)T));
	KD_TRY(t.get(small, 1 + kPlaneWords));
	size_t scan_bytes = 0;
	if (d_out || s.max_planes > 1) {
		// a next cloud is formed; a labels-only call of one round never compacts and needs none of this
		KD_TRY(t.get(buf[0], 3 * N)); KD_TRY(t.get(buf[1], 3 * N));
		KD_TRY(t.get(mapbuf[0], N)); KD_TRY(t.get(mapbuf[1], N));
		KD_TRY(t.get(scan, N + 1));
		KD_TRY(compact_scan_bytes(flag, scan, N, scan_bytes, stream));
		KD_TRY(t.get_bytes(tmp, std::max<size_t>(scan_bytes, 16)));
	}
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	if (d_label) KD_TRY(hipMemsetAsync(d_label, 0xff, sizeof(int32_t) * N, stream));
	const float* cur = d_xyz;
	const int* map = nullptr;                                    // the original index of every point of cur; null: the identity
	int np = n, found = 0, side = 0;
	const dim3 blk(256);
	auto score = [&](const float4* h, int count, unsigned* out) {
		hipLaunchKernelGGL(pl_score_kernel, dim3((unsigned)((np + kPlBlock * kPlPts - 1) / (kPlBlock * kPlPts)), (unsigned)((count + kPlTile - 1) / kPlTile)),
		                   dim3(kPlBlock), 0, stream, cur, np, h, count, s.distance, out);
		return hipGetLastError();
	};
	for (int p = 0; p < s.max_planes && np >= 3; p++) {
		KD_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned) * (size_t)T, stream));
		hipLaunchKernelGGL(pl_hyp_kernel, dim3((T + 255) / 256), blk, 0, stream, cur, np, (unsigned long long)s.seed,
		                   (unsigned long long)p * (unsigned long long)T, T, hyp);
		KD_TRY(hipGetLastError());
		KD_TRY(score(hyp, T, counts));
		hipLaunchKernelGGL(pl_argmax_kernel, dim3(1), blk, 0, stream, counts, T, small);
		KD_TRY(hipGetLastError());
		unsigned long long key = 0ull;
		KD_TRY(hipMemcpyAsync(&key, small, sizeof(key), hipMemcpyDeviceToHost, stream));
		KD_TRY(hipStreamSynchronize(stream));
		const int best_count = (int)(key >> 32), best = (int)(~(unsigned)(key & 0xffffffffull));
		if (best < 0 || best >= T || best_count > np) return hipErrorUnknown;
		if (best_count < std::max(s.min_inliers, 3)) break;
		float4 h[2];
		KD_TRY(hipMemcpyAsync(h, hyp + 2 * (size_t)best, sizeof(h), hipMemcpyDeviceToHost, stream));
		KD_TRY(hipStreamSynchronize(stream));
		PlaneRecord rec;
		rec.normal[0] = h[1].x; rec.normal[1] = h[1].y; rec.normal[2] = h[1].z;
		rec.point[0] = h[0].x; rec.point[1] = h[0].y; rec.point[2] = h[0].z;
		rec.inliers = best_count;
		rec.hypothesis = best;
		rec.refined = 0;
		if (s.refine) {
			float mn[3], mx[3], E = 0.f;
			KD_TRY(launch_cloud_minmax(cur, np, mn, mx, stream));
			for (int k = 0; k < 3; k++) E = std::max(E, mx[k] - mn[k]);
			int e = 0;
			std::frexp(E, &e);
			KD_TRY(hipMemsetAsync(small + 1, 0, sizeof(unsigned long long) * kPlaneWords, stream));
			hipLaunchKernelGGL(pl_moment_kernel, dim3((np + 255) / 256), blk, 0, stream, cur, np, h[0], h[1], s.distance, mn[0], mn[1], mn[2], 31 - e, small + 1);
			KD_TRY(hipGetLastError());
			unsigned long long w[kPlaneWords];
			KD_TRY(hipMemcpyAsync(w, small + 1, sizeof(w), hipMemcpyDeviceToHost, stream));
			KD_TRY(hipStreamSynchronize(stream));
			float rn[3], rp[3];
			if (plane_refit(w, mn, e, rn, rp)) {
				// the refit plane takes the place of hypothesis 0 (the round's hypotheses are done with) and is scored by the same kernel
				const float4 r[2] = {make_float4(rp[0], rp[1], rp[2], 0.f), make_float4(rn[0], rn[1], rn[2], 0.f)};
				unsigned cnt = 0u;
				KD_TRY(hipMemcpyAsync(hyp, r, sizeof(r), hipMemcpyHostToDevice, stream));
				KD_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned), stream));
				KD_TRY(score(hyp, 1, counts));
				KD_TRY(hipMemcpyAsync(&cnt, counts, sizeof(cnt), hipMemcpyDeviceToHost, stream));
				KD_TRY(hipStreamSynchronize(stream));
				if (cnt > (unsigned)np) return hipErrorUnknown;
				if ((int)cnt >= rec.inliers) {
					for (int k = 0; k < 3; k++) { rec.normal[k] = rn[k]; rec.point[k] = rp[k]; }
					rec.inliers = (int)cnt;
					rec.refined = 1;
					h[0] = r[0]; h[1] = r[1];
				}
			}
		}
		rec.d = plane::offset(rec.normal, rec.point);
		planes[found] = rec;
		hipLaunchKernelGGL(pl_label_kernel, dim3((np + 255) / 256), blk, 0, stream, cur, np, h[0], h[1], s.distance, map, found, d_label, flag);
		KD_TRY(hipGetLastError());
		found++;
		if (!d_out && p + 1 == s.max_planes) { np -= rec.inliers; break; }      // only labels are wanted and no round follows: no next cloud
		// the next round's cloud and its index map: round 0 writes the positions themselves, the later rounds carry the map as the label column
		int m = -1;
		KD_TRY(compact_tail(cur, np, flag, scan, tmp, scan_bytes, map, buf[side], map ? nullptr : mapbuf[side], map ? mapbuf[side] : nullptr, &m, stream));
		KD_TRY(hipStreamSynchronize(stream));
		if (m != np - rec.inliers) return hipErrorUnknown;
		cur = buf[side]; map = mapbuf[side]; np = m;
		side ^= 1;
	}
	if (d_out && np > 0) {
		KD_TRY(hipMemcpyAsync(d_out, cur, sizeof(float) * 3 * (size_t)np, hipMemcpyDeviceToDevice, stream));
		if (d_index) {
			if (map) KD_TRY(hipMemcpyAsync(d_index, map, sizeof(int) * (size_t)np, hipMemcpyDeviceToDevice, stream));
			else hipLaunchKernelGGL(so_iota_kernel, dim3((np + 255) / 256), blk, 0, stream, d_index, np);
			KD_TRY(hipGetLastError());
		}
	}
	*n_planes = found;
	*m_out = np;
	return end_and_drain(ev_end, stream);
}

// ------------------------------------------------------------------------------------------------
// RANSAC pose estimation from correspondences on the device (host twin: ransac_pose_host, kdtree.cpp).  The gather kernel packs
// the correspondences once; the hypothesis kernel (one thread per hypothesis: the draw, the pre-rejection and the fp64 pose, device.hpp's
// text); the score kernel (all correspondences x all hypotheses, integer counts); the keys (count << 32) | ~t sorted descending by rocPRIM;
// the first max_poses keys and their poses to the host; with refine the integer-moment kernel over (pose, correspondence), 200 bytes per
// pose to the host, ransac_pose_refit there, the score kernel once more on the refit poses; the mask kernel for pose 0.
// ------------------------------------------------------------------------------------------------
static_assert(kRpTile == kRpBlock && kRpTile % 64 == 0, "one thread loads one hypothesis of the tile; a wave keeps 64 counts at a time");
constexpr int kRpSpan = kRpBlock * kRpPts;                     // correspondences of a score workgroup

// ps[j] = (source point of correspondence j, 0), pt[j] = (its target point, 0); a slot j >= M (the arrays are padded to whole spans) holds
// NaN: never an inlier
__global__ void rp_gather_kernel(const float* __restrict__ src, const float* __restrict__ tgt, const int32_t* __restrict__ corr, int M, int slots,
                                 float4* __restrict__ ps, float4* __restrict__ pt)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= slots) return;
	const float nan = __int_as_float(0x7fc00000);
	float4 s = make_float4(nan, nan, nan, 0.f), m = s;
	if (j < M) {
		const size_t a = (size_t)corr[2 * (size_t)j], b = (size_t)corr[2 * (size_t)j + 1];
		s = make_float4(src[3 * a], src[3 * a + 1], src[3 * a + 2], 0.f);
		m = make_float4(tgt[3 * b], tgt[3 * b + 1], tgt[3 * b + 2], 0.f);
	}
	ps[j] = s;
	pt[j] = m;
}

// hyp[3 t + a] = (R_a0, R_a1, R_a2, t_a) of hypothesis t; a rejected or degenerate hypothesis is NaN throughout, against which no pair is an
// inlier: it scores 0
__global__ void __launch_bounds__(256) rp_hyp_kernel(const float4* __restrict__ ps, const float4* __restrict__ pt, int M, unsigned long long seed, int T,
                                                     float sigma, float4* __restrict__ hyp)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= T) return;
	uint32_t a, b, c;
	plane::draw(seed, (unsigned long long)t, (uint32_t)M, &a, &b, &c);
	const float4 qa = ps[a], qb = ps[b], qc = ps[c], ma = pt[a], mb = pt[b], mc = pt[c];
	const float sa[3] = {qa.x, qa.y, qa.z}, sb[3] = {qb.x, qb.y, qb.z}, sc[3] = {qc.x, qc.y, qc.z};
	const float ta[3] = {ma.x, ma.y, ma.z}, tb[3] = {mb.x, mb.y, mb.z}, tc[3] = {mc.x, mc.y, mc.z};
	float R[9], tr[3];
	bool ok = sigma > 0.f ? pose::triple_ok(sa, sb, sc, ta, tb, tc, sigma) : true;
	ok = ok && pose::of_triple(sa, sb, sc, ta, tb, tc, R, tr);
	const float nan = __int_as_float(0x7fc00000);
#pragma unroll
	for (int r = 0; r < 3; r++)
		hyp[3 * (size_t)t + r] = ok ? make_float4(R[3 * r], R[3 * r + 1], R[3 * r + 2], tr[r]) : make_float4(nan, nan, nan, nan);
}

// Workgroup (bx, by): the kRpSpan correspondences from bx * kRpSpan against the hypotheses by * kRpTile ...  A lane keeps kRpPts
// correspondences in registers; the tile's poses sit in LDS and are read wave-uniformly as three 128-bit words; per hypothesis and
// correspondence the float pair, a ballot and a popcount of its 64-bit mask.  The wave's count of hypothesis j0 + jj stays with lane jj, so
// LDS sees one atomic per lane per 64 hypotheses, and global memory one atomic per hypothesis per workgroup (pl_score_kernel's shape)
__global__ void __launch_bounds__(kRpBlock) rp_score_kernel(const float4* __restrict__ ps, const float4* __restrict__ pt, const float4* __restrict__ hyp, int T,
                                                            float d2max, unsigned* __restrict__ counts)
{
	__shared__ float4 s_r0[kRpTile], s_r1[kRpTile], s_r2[kRpTile];
	__shared__ unsigned s_cnt[kRpTile];
	const int tid = threadIdx.x, lane = tid & 63;
	const int t0 = blockIdx.y * kRpTile;
	const float nan = __int_as_float(0x7fc00000);
	{
		const int t = t0 + tid;
		float4 r0 = make_float4(nan, nan, nan, nan), r1 = r0, r2 = r0;
		if (t < T) { r0 = hyp[3 * (size_t)t]; r1 = hyp[3 * (size_t)t + 1]; r2 = hyp[3 * (size_t)t + 2]; }
		s_r0[tid] = r0; s_r1[tid] = r1; s_r2[tid] = r2;
		s_cnt[tid] = 0u;
	}
	float sx[kRpPts], sy[kRpPts], sz[kRpPts], mx[kRpPts], my[kRpPts], mz[kRpPts];
	const size_t base = (size_t)blockIdx.x * (size_t)kRpSpan;    // the packed arrays hold whole spans: no slot is past their end
#pragma unroll
	for (int k = 0; k < kRpPts; k++) {
		const float4 s = ps[base + (size_t)(k * kRpBlock + tid)], m = pt[base + (size_t)(k * kRpBlock + tid)];
		sx[k] = s.x; sy[k] = s.y; sz[k] = s.z; mx[k] = m.x; my[k] = m.y; mz[k] = m.z;
	}
	__syncthreads();
	const int live = min(kRpTile, T - t0);                      // the tile's hypotheses that exist
	for (int j0 = 0; j0 < live; j0 += 64) {
		unsigned mine = 0u;
		const int jn = min(64, live - j0);                      // wave-uniform; a lane past it keeps 0 (the refit's re-score has few poses)
		for (int jj = 0; jj < jn; jj++) {
			const float4 r0 = s_r0[j0 + jj], r1 = s_r1[j0 + jj], r2 = s_r2[j0 + jj];
			unsigned c = 0u;
#pragma unroll
			for (int k = 0; k < kRpPts; k++) {
				const float e0 = pose::residual(r0.x, r0.y, r0.z, r0.w, sx[k], sy[k], sz[k], mx[k]);
				const float e1 = pose::residual(r1.x, r1.y, r1.z, r1.w, sx[k], sy[k], sz[k], my[k]);
				const float e2 = pose::residual(r2.x, r2.y, r2.z, r2.w, sx[k], sy[k], sz[k], mz[k]);
				c += (unsigned)__popcll(__ballot(pose::within(e0, e1, e2, d2max)));
			}
			mine = lane == jj ? c : mine;
		}
		if (mine) atomicAdd(&s_cnt[j0 + lane], mine);
	}
	__syncthreads();
	if (t0 + tid < T && s_cnt[tid]) atomicAdd(&counts[t0 + tid], s_cnt[tid]);
}

__global__ void rp_key_kernel(const unsigned* __restrict__ counts, int T, unsigned long long* __restrict__ keys)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < T) keys[t] = ((unsigned long long)counts[t] << 32) | (unsigned long long)(~(unsigned)t);
}

// the poses of the K largest keys, in their order: out[3 i + r] = hyp[3 t_i + r]
__global__ void rp_take_kernel(const unsigned long long* __restrict__ sorted, int K, int T, const float4* __restrict__ hyp, float4* __restrict__ out)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= 3 * K) return;
	const unsigned t = ~(unsigned)(sorted[i / 3] & 0xffffffffull);
	const float nan = __int_as_float(0x7fc00000);
	out[i] = t < (unsigned)T ? hyp[3 * (size_t)t + (size_t)(i % 3)] : make_float4(nan, nan, nan, nan);
}

// the refit's 25 integer words of pose blockIdx.y over its inliers: one thread per correspondence, wave-level sums, then 64-bit atomics
// (pl_moment_kernel's style).  q < 2^31 on both sides, so a product has 62 bits and every word of at most 2^28 correspondences stays below 2^60
__global__ void __launch_bounds__(256) rp_moment_kernel(const float4* __restrict__ ps, const float4* __restrict__ pt, int M, const float4* __restrict__ poses,
                                                        float d2max, float4 mns, float4 mnt, int shs, int sht, unsigned long long* __restrict__ words)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	const float4 r0 = poses[3 * blockIdx.y], r1 = poses[3 * blockIdx.y + 1], r2 = poses[3 * blockIdx.y + 2];
	unsigned long long w[kRansacPoseWords];
#pragma unroll
	for (int k = 0; k < kRansacPoseWords; k++) w[k] = 0ull;
	if (j < M) {
		const float4 s = ps[j], m = pt[j];
		const float e0 = pose::residual(r0.x, r0.y, r0.z, r0.w, s.x, s.y, s.z, m.x), e1 = pose::residual(r1.x, r1.y, r1.z, r1.w, s.x, s.y, s.z, m.y),
		            e2 = pose::residual(r2.x, r2.y, r2.z, r2.w, s.x, s.y, s.z, m.z);
		if (pose::within(e0, e1, e2, d2max)) {
			const unsigned long long qs[3] = {(unsigned long long)llrint(ldexp((double)(s.x - mns.x), shs)), (unsigned long long)llrint(ldexp((double)(s.y - mns.y), shs)),
			                                  (unsigned long long)llrint(ldexp((double)(s.z - mns.z), shs))};
			const unsigned long long qt[3] = {(unsigned long long)llrint(ldexp((double)(m.x - mnt.x), sht)), (unsigned long long)llrint(ldexp((double)(m.y - mnt.y), sht)),
			                                  (unsigned long long)llrint(ldexp((double)(m.z - mnt.z), sht))};
			w[0] = 1ull;
#pragma unroll
			for (int a = 0; a < 3; a++) {
				w[1 + a] = qs[a]; w[4 + a] = qt[a];
#pragma unroll
				for (int b = 0; b < 3; b++) {
					const unsigned long long p = qt[a] * qs[b];
					w[7 + 3 * a + b] = p >> 32; w[16 + 3 * a + b] = p & 0xffffffffull;
				}
			}
		}
	}
#pragma unroll
	for (int k = 0; k < kRansacPoseWords; k++)
		for (int off = 32; off; off >>= 1) w[k] += shfl_xor64(w[k], off);
	if ((threadIdx.x & 63) == 0 && w[0]) {
#pragma unroll
		for (int k = 0; k < kRansacPoseWords; k++) atomicAdd(words + (size_t)blockIdx.y * kRansacPoseWords + k, w[k]);
	}
}

// the pair's verdict of every correspondence under one pose
__global__ void rp_mask_kernel(const float4* __restrict__ ps, const float4* __restrict__ pt, int M, float4 r0, float4 r1, float4 r2, float d2max,
                               unsigned char* __restrict__ inlier)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= M) return;
	const float4 s = ps[j], m = pt[j];
	inlier[j] = pose::within(pose::residual(r0.x, r0.y, r0.z, r0.w, s.x, s.y, s.z, m.x), pose::residual(r1.x, r1.y, r1.z, r1.w, s.x, s.y, s.z, m.y),
	                         pose::residual(r2.x, r2.y, r2.z, r2.w, s.x, s.y, s.z, m.z), d2max) ? 1 : 0;
}

hipError_t launch_ransac_pose(const float* d_src, const float* d_tgt, const int32_t* d_corr, int M, const RansacPoseSelect& s, const RansacPoseFrame& fs,
                              const RansacPoseFrame& ft, RansacPoseRecord* poses, int* n_poses, unsigned char* d_inlier, hipStream_t stream,
                              hipEvent_t ev_begin, hipEvent_t ev_end)
{
	if (M < 3 || !d_src || !d_tgt || !d_corr || !poses || !n_poses) return hipErrorInvalidValue;
	if (s.iterations < 1 || s.iterations > kRansacPoseMaxIterations || s.max_poses < 1 || s.max_poses > kRansacPoseMaxPoses) return hipErrorInvalidValue;
	const int T = s.iterations, K = std::min(s.max_poses, T);
	const int spans = (M + kRpSpan - 1) / kRpSpan, slots = spans * kRpSpan;
	const float d2max = s.distance * s.distance;
	float4 *ps = nullptr, *pt = nullptr, *hyp = nullptr, *top = nullptr;   // top: the K returned poses, then the K refit poses
	unsigned* counts = nullptr;
	unsigned long long *keys = nullptr, *sorted = nullptr, *words = nullptr;
	void* tmp = nullptr;
	size_t sort_bytes = 0;
	Temps t;
	KD_TRY(t.get(ps, (size_t)slots)); KD_TRY(t.get(pt, (size_t)slots));
	KD_TRY(t.get(hyp, 3 * (size_t)T));
	KD_TRY(t.get(top, 6 * (size_t)kRansacPoseMaxPoses));
	KD_TRY(t.get(counts, (size_t)T));
	KD_TRY(t.get(keys, (size_t)T)); KD_TRY(t.get(sorted, (size_t)T));
	KD_TRY(t.get(words, (size_t)kRansacPoseMaxPoses * kRansacPoseWords));
	KD_TRY(rocprim::radix_sort_keys_desc(nullptr, sort_bytes, keys, sorted, (size_t)T, 0, 64, stream));
	KD_TRY(t.get_bytes(tmp, std::max<size_t>(sort_bytes, 16)));
	if (ev_begin) KD_TRY(hipEventRecord(ev_begin, stream));
	const dim3 blk(256);
	auto score = [&](const float4* h, int count, unsigned* out) {
		hipLaunchKernelGGL(rp_score_kernel, dim3((unsigned)spans, (unsigned)((count + kRpTile - 1) / kRpTile)), dim3(kRpBlock), 0, stream, ps, pt, h, count, d2max,
		                   out);
		return hipGetLastError();
	};
	hipLaunchKernelGGL(rp_gather_kernel, dim3((slots + 255) / 256), blk, 0, stream, d_src, d_tgt, d_corr, M, slots, ps, pt);
	KD_TRY(hipGetLastError());
	KD_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned) * (size_t)T, stream));
	hipLaunchKernelGGL(rp_hyp_kernel, dim3((T + 255) / 256), blk, 0, stream, ps, pt, M, (unsigned long long)s.seed, T, s.edge_similarity, hyp);
	KD_TRY(hipGetLastError());
	KD_TRY(score(hyp, T, counts));
	hipLaunchKernelGGL(rp_key_kernel, dim3((T + 255) / 256), blk, 0, stream, counts, T, keys);
	KD_TRY(hipGetLastError());
	KD_TRY(rocprim::radix_sort_keys_desc(tmp, sort_bytes, keys, sorted, (size_t)T, 0, 64, stream));
	hipLaunchKernelGGL(rp_take_kernel, dim3((3 * K + 255) / 256), blk, 0, stream, sorted, K, T, hyp, top);
	KD_TRY(hipGetLastError());
	unsigned long long key[kRansacPoseMaxPoses];
	float4 h[3 * kRansacPoseMaxPoses];
	KD_TRY(hipMemcpyAsync(key, sorted, sizeof(unsigned long long) * (size_t)K, hipMemcpyDeviceToHost, stream));
	KD_TRY(hipMemcpyAsync(h, top, sizeof(float4) * 3 * (size_t)K, hipMemcpyDeviceToHost, stream));
	KD_TRY(hipStreamSynchronize(stream));
	int found = 0;
	const int floor_count = std::max(s.min_inliers, 3);
	for (; found < K; found++) {
		const long long cnt = (long long)(key[found] >> 32);
		const unsigned best = ~(unsigned)(key[found] & 0xffffffffull);
		if (best >= (unsigned)T || cnt > (long long)M) return hipErrorUnknown;
		if (cnt < (long long)floor_count) break;
		RansacPoseRecord& rec = poses[found];
		for (int r = 0; r < 3; r++) {
			const float4 row = h[3 * found + r];
			rec.R[3 * r] = row.x; rec.R[3 * r + 1] = row.y; rec.R[3 * r + 2] = row.z; rec.t[r] = row.w;
		}
		rec.inliers = (int32_t)cnt;
		rec.hypothesis = (int32_t)best;
		rec.refined = 0;
	}
	if (s.refine && found > 0) {
		KD_TRY(hipMemsetAsync(words, 0, sizeof(unsigned long long) * (size_t)found * kRansacPoseWords, stream));
		hipLaunchKernelGGL(rp_moment_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)found), blk, 0, stream, ps, pt, M, top, d2max,
		                   make_float4(fs.mn[0], fs.mn[1], fs.mn[2], 0.f), make_float4(ft.mn[0], ft.mn[1], ft.mn[2], 0.f), 31 - fs.e, 31 - ft.e, words);
		KD_TRY(hipGetLastError());
		unsigned long long w[kRansacPoseMaxPoses * kRansacPoseWords];
		KD_TRY(hipMemcpyAsync(w, words, sizeof(unsigned long long) * (size_t)found * kRansacPoseWords, hipMemcpyDeviceToHost, stream));
		KD_TRY(hipStreamSynchronize(stream));
		const float nan = std::nanf("");
		float4 r[3 * kRansacPoseMaxPoses];
		for (int i = 0; i < found; i++) {
			float R[9], tr[3];
			const bool ok = ransac_pose_refit(w + (size_t)i * kRansacPoseWords, fs, ft, R, tr);
			for (int a = 0; a < 3; a++) r[3 * i + a] = ok ? make_float4(R[3 * a], R[3 * a + 1], R[3 * a + 2], tr[a]) : make_float4(nan, nan, nan, nan);
		}
		// the refit poses are scored by the same kernel as `found` hypotheses; a refit that does not exist is NaN and counts 0
		unsigned cnt[kRansacPoseMaxPoses];
		float4* refit = top + 3 * (size_t)kRansacPoseMaxPoses;
		KD_TRY(hipMemcpyAsync(refit, r, sizeof(float4) * 3 * (size_t)found, hipMemcpyHostToDevice, stream));
		KD_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned) * (size_t)found, stream));
		KD_TRY(score(refit, found, counts));
		KD_TRY(hipMemcpyAsync(cnt, counts, sizeof(unsigned) * (size_t)found, hipMemcpyDeviceToHost, stream));
		KD_TRY(hipStreamSynchronize(stream));
		for (int i = 0; i < found; i++) {
			if (cnt[i] > (unsigned)M) return hipErrorUnknown;
			RansacPoseRecord& rec = poses[i];
			if (r[3 * i].x == r[3 * i].x && (int32_t)cnt[i] >= rec.inliers) {
				for (int a = 0; a < 3; a++) {
					const float4 row = r[3 * i + a];
					rec.R[3 * a] = row.x; rec.R[3 * a + 1] = row.y; rec.R[3 * a + 2] = row.z; rec.t[a] = row.w;
				}
				rec.inliers = (int32_t)cnt[i];
				rec.refined = 1;
			}
		}
	}
	if (d_inlier) {
		if (found > 0) {
			const RansacPoseRecord& p = poses[0];
			hipLaunchKernelGGL(rp_mask_kernel, dim3((M + 255) / 256), blk, 0, stream, ps, pt, M, make_float4(p.R[0], p.R[1], p.R[2], p.t[0]),
			                   make_float4(p.R[3], p.R[4], p.R[5], p.t[1]), make_float4(p.R[6], p.R[7], p.R[8], p.t[2]), d2max, d_inlier);
			KD_TRY(hipGetLastError());
		} else {
			KD_TRY(hipMemsetAsync(d_inlier, 0, (size_t)M, stream));
		}
	}
	*n_poses = found;
	return end_and_drain(ev_end, stream);
}

}  // namespace goicp
