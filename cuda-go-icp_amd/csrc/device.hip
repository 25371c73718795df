// HIP kernels of the MI355X Go-ICP engine (gfx950 / CDNA4, wave64).  Compiled with
// -ffp-contract=off: every per-point value follows the reference CPU path's float/double operation
// order (no FMA contraction), so distances, clamps and squares are bit-identical to
// src/goicp/jly_goicp.cpp / jly_3ddt.cpp / jly_icp3d.hpp; only the order of the sums differs.
//
// Kernels
//   bounds_kernel        (a) BnB cube bounds: rotate + translate the source cloud, gather the 3-D
//                        Euclidean distance transform, subtract uncertainty radii, sum of squares.
//                        16 B (ub pass) / 20 B (lb pass) algorithmic per point; sibling fast path.
//   bounds_finalize      fixed-order sum of the per-chunk partials (deterministic, no float atomics)
//   bounds_trim_kernel   trimmed form: exact k-th smallest residual per cube by radix select
//   icp_pass_kernel      (b) one ICP correspondence pass: transform, exact 1-NN (four queries per
//                        wavefront over a 64-ary box hierarchy, DT-seeded bound), pivoted sums
//   icp_finalize_update  fixed-order double-precision reduction + the rest of the ICP loop body
//                        (convergence test, SVD, pose update) on the device-resident state
//   icp_nn/select/accum  trimmed ICP: NN of every point, radix select of the num nearest, sums
//   transform_kernel     rigid transform apply
//   nn_query_kernel      1-NN operator for arbitrary queries
//   knn_query_kernel     exact k-NN operator (k <= 32), ascending (d2, index)
//   normal_build_kernel  target normals: k-NN, fp64 covariance, smallest eigenvector (opt-in point-to-plane ICP)
//   icp_plane_pass_kernel / icp_plane_finalize   point-to-plane ICP iteration: the same walk, 28 fixed-point sums, 6x6 solve
//   dt_*               exact Euclidean DT build (seed, three separable min-plus passes, sqrt/scale)
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cmath>

#include "device.hpp"

namespace goicp {

// ------------------------------------------------------------------------------------------------
// wave64 helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

// XCD-aware bijective block remap: blocks b and b+8 share an XCD (round-robin dispatch), so give
// each XCD a contiguous slice of the logical grid -> neighbouring cube groups (neighbouring DT
// lines) meet in one L2.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int nb)
{
	int q = nb >> 3, r = nb & 7, xcd = bid & 7;
	return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// ------------------------------------------------------------------------------------------------
// DT lookup = DT3D::Distance (jly_3ddt.cpp:981-1026), nearest voxel with int(x+0.5) truncation
// ------------------------------------------------------------------------------------------------
// layout 2 (opt-in, Params::bounds_fp16): the bricked grid in IEEE half precision -- a 4x4x4 brick is then ONE 128-byte
// line instead of two, which halves the distinct lines a 64-lane gather touches (the cost the bounds kernel is bound
// by).  Values are rounded toward zero when the copy is made, so every lower bound stays a valid lower bound; upper
// bounds come out low by at most 2^-10 relative.  Index arithmetic is the bricked layout's.
__device__ __forceinline__ float half_bits_to_float(unsigned short h)
{
	return __half2float(__ushort_as_half(h));
}
// element e of a half grid through a 4-byte load of the aligned pair that holds it (measured: 2-byte gathers run at a
// fraction of the dword rate -- the S2 launch took 80.6 ms with global_load_ushort against 53.8 ms in fp32)
__device__ __forceinline__ float half_fetch(const float* grid, unsigned e)
{
	const unsigned w = *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(grid) + (size_t)((e >> 1) << 2));
	return half_bits_to_float((unsigned short)((e & 1u) ? (w >> 16) : (w & 0xffffu)));
}

template <int LAYOUT>
__device__ __forceinline__ float dt_fetch(const DtDesc& dt, int x, int y, int z)
{
	// 24-bit multiplies (full rate) and a 32-bit byte offset from a scalar base: V <= 640 keeps
	// every offset below 2^32 (engine.cpp enforces it)
	unsigned e;
	if (LAYOUT == 0) {
		e = __umul24(__umul24((unsigned)z, (unsigned)dt.V) + (unsigned)y, (unsigned)dt.V) + (unsigned)x;
	} else {
		const unsigned b = __umul24(__umul24((unsigned)z >> 2, (unsigned)dt.VB) + ((unsigned)y >> 2), (unsigned)dt.VB) + ((unsigned)x >> 2);
		e = (b << 6) | (brick_z((unsigned)z) | brick_y((unsigned)y) | brick_x((unsigned)x));
	}
	if (LAYOUT == 2) return half_fetch(dt.grid, e);
	return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(dt.grid) + (size_t)(e << 2));
}

// voxel index of one coordinate: the reference computes int((double(q) - min)*scale + 0.5) in double
// (jly_3ddt.cpp:984-986).  Fast path: the same expression in float (1 sub + 1 fma) is within
// eps(F) = c1 + c2*|F| of the exact value (rounding of min, scale, the difference and the fma;
// DtDesc.c1/c2 are computed on the host from the grid geometry); whenever F is farther than eps
// from the nearest integer, truncating F gives the reference's index.  Otherwise -- a few lanes
// in 10^4 -- the caller recomputes in double.  Result: bit-identical indices at ~1/3 of the cost.
__device__ __forceinline__ int voxel_fast(float q, float mn, float scale, float c1, float c2, bool& risky)
{
	const float F = __fmaf_rn(q - mn, scale, 0.5f);
	risky = risky || (fabsf(F - rintf(F)) <= __fmaf_rn(fabsf(F), c2, c1));
	return (int)F;
}

// reference expression (jly_3ddt.cpp:984-986), taken by the few lanes in 10^4 whose float index is not
// provably right.  The empty asm keeps the caller's `if (risky)` a real branch: left to itself the
// compiler if-converts it and puts the five fp64 instructions of every index on every lane (measured:
// 30 of the 255 VALU instructions per point of the sibling path, at half rate).
__device__ __forceinline__ int voxel_exact(float q, double mn, double scale)
{
	__asm__ volatile("");
	return (int)(((double)q - mn) * scale + 0.5);
}

template <int LAYOUT>
__device__ __forceinline__ float dt_distance(const DtDesc& dt, float qx, float qy, float qz)
{
	bool risky = false;
	int x = voxel_fast(qx, dt.xmin_f, dt.scale_f, dt.c1, dt.c2, risky);
	int y = voxel_fast(qy, dt.ymin_f, dt.scale_f, dt.c1, dt.c2, risky);
	int z = voxel_fast(qz, dt.zmin_f, dt.scale_f, dt.c1, dt.c2, risky);
	if (risky) {
		// double index math exactly as the reference: (x - xMin)*scale + 0.5, truncate
		x = voxel_exact(qx, dt.xmin, dt.scale);
		y = voxel_exact(qy, dt.ymin, dt.scale);
		z = voxel_exact(qz, dt.zmin, dt.scale);
	}
	const int V = dt.V;
	if ((unsigned)x < (unsigned)V && (unsigned)y < (unsigned)V && (unsigned)z < (unsigned)V)
		return dt_fetch<LAYOUT>(dt, x, y, z);
	// outside the grid: clamp to the face and add the overshoot (in voxels) / scale
	float a = 0.f, b = 0.f, c = 0.f;
	if (x < 0) { a = (float)x; x = 0; } else if (x >= V) { a = (float)(x - V + 1); x = V - 1; }
	if (y < 0) { b = (float)y; y = 0; } else if (y >= V) { b = (float)(y - V + 1); y = V - 1; }
	if (z < 0) { c = (float)z; z = 0; } else if (z >= V) { c = (float)(z - V + 1); z = V - 1; }
	// sqrt(a^2+b^2+c^2)/scale: a, b, c are small integers, so the term is a function of the integer
	// s = a^2+b^2+c^2 only.  DtDesc.overshoot[s] holds (double)sqrtf(s)/scale computed on the host with
	// the same operations (bit-identical), which replaces a float sqrt and an fp64 division on this path.
	const int si = (int)(a * a + b * b + c * c);
	const double ext = si < dt.n_overshoot ? dt.overshoot[si] : (double)__fsqrt_rn(a * a + b * b + c * c) / dt.scale;
	return (float)(ext + (double)dt_fetch<LAYOUT>(dt, x, y, z));
}

// Per-axis part of a voxel's element offset.  Both layouts are separable: offset = fx(x)+fy(y)+fz(z);
// an out-of-grid index contributes kOutside (>= 2^30 > any in-grid sum, and three of them do not wrap),
// so one unsigned compare of the sum tells whether the fast fetch is valid.
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr unsigned kOutside = 0x40000000u;
template <int LAYOUT, int AXIS>
__device__ __forceinline__ unsigned axis_offset(const DtDesc& dt, int i)
{
	if ((unsigned)i >= (unsigned)dt.V) return kOutside;
	const unsigned u = (unsigned)i;
	if (LAYOUT == 0) return AXIS == 0 ? u : (AXIS == 1 ? __umul24(u, (unsigned)dt.V) : __umul24(u, (unsigned)(dt.V * dt.V)));
	const unsigned hi = u >> 2;
	if (AXIS == 0) return (hi << 6) | brick_x(u);
	if (AXIS == 1) return (__umul24(hi, (unsigned)dt.VB) << 6) | brick_y(u);
	return (__umul24(hi, (unsigned)(dt.VB * dt.VB)) << 6) | brick_z(u);
}

// the 8 cube records of workgroup `group`: read from the batch, or derived from one expansion record with
// the search driver's own float operations (engine.cpp / jly_goicp.cpp:262-273: w' = w/2, corner +
// bit*w', centre = corner + w'/2, delta = float(sqrt3/2 * double(w')))
__device__ __forceinline__ void load_group(const CubeRec* __restrict__ cubes, const ParentRec* __restrict__ parents, int group, int B,
                                           CubeRec cr[kGroup])
{
	if (parents) {
		const ParentRec pr = parents[group];
		const float w = pr.w / 2;
		const float delta = (float)(1.732050808 / 2.0 * (double)w);
#pragma unroll
		for (int c = 0; c < kGroup; c++) {
			const float cx = pr.x + (float)(c & 1) * w, cy = pr.y + (float)((c >> 1) & 1) * w, cz = pr.z + (float)((c >> 2) & 1) * w;
			cr[c].tx = cx + w / 2; cr[c].ty = cy + w / 2; cr[c].tz = cz + w / 2;
			cr[c].delta = delta; cr[c].coeff = pr.coeff; cr[c].rot = pr.rot;
		}
	} else {
		const int c0 = group * kGroup;
#pragma unroll
		for (int c = 0; c < kGroup; c++) cr[c] = cubes[c0 + c < B ? c0 + c : B - 1];
	}
}

// The clamped residuals max(DT(R p + t_c) - rho, 0) of one point under the 8 children of one expansion
// (one rotation, per axis two translation values): 6 voxel indices instead of 24.  Every value is the same
// float expression as in the generic per-cube path, so the results are bit-identical.
struct SiblingSet { float tx0, tx1, ty0, ty1, tz0, tz1; };
// rp = R p already formed (xyz)
template <int LAYOUT>
__device__ __forceinline__ void sibling_residuals_rotated(const DtDesc& dt, const float4& rp, const SiblingSet& t, float rho, float m[kGroup]);
template <int LAYOUT>
__device__ __forceinline__ void sibling_residuals(const DtDesc& dt, const Rot9& R0, const SiblingSet& t, const float4& p, float rho,
                                                  float m[kGroup])
{
	const float rx = R0.r[0] * p.x + R0.r[1] * p.y + R0.r[2] * p.z;
	const float ry = R0.r[3] * p.x + R0.r[4] * p.y + R0.r[5] * p.z;
	const float rz = R0.r[6] * p.x + R0.r[7] * p.y + R0.r[8] * p.z;
	sibling_residuals_rotated<LAYOUT>(dt, make_float4(rx, ry, rz, p.w), t, rho, m);
}
template <int LAYOUT>
__device__ __forceinline__ void sibling_residuals_rotated(const DtDesc& dt, const float4& rp, const SiblingSet& t, float rho, float m[kGroup])
{
	const float rx = rp.x, ry = rp.y, rz = rp.z;
	const float qx[2] = {rx + t.tx0, rx + t.tx1}, qy[2] = {ry + t.ty0, ry + t.ty1}, qz[2] = {rz + t.tz0, rz + t.tz1};
	bool risky = false;
	int ix[2], iy[2], iz[2];
#pragma unroll
	for (int k = 0; k < 2; k++) {
		ix[k] = voxel_fast(qx[k], dt.xmin_f, dt.scale_f, dt.c1, dt.c2, risky);
		iy[k] = voxel_fast(qy[k], dt.ymin_f, dt.scale_f, dt.c1, dt.c2, risky);
		iz[k] = voxel_fast(qz[k], dt.zmin_f, dt.scale_f, dt.c1, dt.c2, risky);
	}
	if (risky) {
#pragma unroll
		for (int k = 0; k < 2; k++) {
			ix[k] = voxel_exact(qx[k], dt.xmin, dt.scale);
			iy[k] = voxel_exact(qy[k], dt.ymin, dt.scale);
			iz[k] = voxel_exact(qz[k], dt.zmin, dt.scale);
		}
	}
	const unsigned fx[2] = {axis_offset<LAYOUT, 0>(dt, ix[0]), axis_offset<LAYOUT, 0>(dt, ix[1])};
	const unsigned fy[2] = {axis_offset<LAYOUT, 1>(dt, iy[0]), axis_offset<LAYOUT, 1>(dt, iy[1])};
	const unsigned fz[2] = {axis_offset<LAYOUT, 2>(dt, iz[0]), axis_offset<LAYOUT, 2>(dt, iz[1])};
#pragma unroll
	for (int c = 0; c < kGroup; c++) {
		const unsigned e = fx[c & 1] + fy[(c >> 1) & 1] + fz[(c >> 2) & 1];
		float v;
		if (e < kOutside) {
			if (LAYOUT == 2) v = half_fetch(dt.grid, e);
			else v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(dt.grid) + (size_t)(e << 2));
		}
		else v = dt_distance<LAYOUT>(dt, qx[c & 1], qy[(c >> 1) & 1], qz[(c >> 2) & 1]);   // clamp + overshoot extension
		v = v - rho;
		m[c] = v < 0.f ? 0.f : v;
	}
}
// do the 8 records describe the children of one expansion?  (jly_goicp.cpp:267-273: corner + bit*w + w/2)
__device__ __forceinline__ bool is_sibling_set(const CubeRec cr[kGroup])
{
	bool sib = true;
#pragma unroll
	for (int c = 0; c < kGroup; c++)
		sib = sib && cr[c].rot == cr[0].rot && cr[c].tx == cr[c & 1].tx && cr[c].ty == cr[c & 2].ty && cr[c].tz == cr[c & 4].tz &&
		      cr[c].delta == cr[0].delta && cr[c].coeff == cr[0].coeff;
	return sib;
}

// ------------------------------------------------------------------------------------------------
// (a) cube bounds
// ------------------------------------------------------------------------------------------------
// grid: groups*chunks blocks of 256 threads.  A block owns kGroup consecutive cubes (the siblings
// of one BnB expansion: same rotation, neighbouring translations -> neighbouring DT voxels) and a
// contiguous chunk of the (k-d-ordered) source cloud; each point is loaded once (16 B) and
// reused for the 8 cubes.
//
// The lean sibling path over the points [p0, p1) of a chunk (round 3; fp32 grids that fit the Infinity Cache): one exactness test per
// point on the smallest margin of the six indices; a wavefront whose indices are all inside the grid fetches without per-child checks;
// the eight children are accumulated as four x-sibling pairs in packed fp32 -- the same operations per element as the checked path,
// bit-identical bounds.  NP = 2: the SAME expansion listed by both searches of a rotation child (coeff[0] = the lower-bound pass's
// coefficient, coeff[1] = 0 of the upper-bound pass): one gather serves both, only the subtraction of the rotation radius and the
// sums are per pass -- each pass's sums see exactly the operations of a separate evaluation.
// LAST_ZERO: coeff[NP - 1] is known to be 0 (the upper-bound pass, jly_goicp.cpp:284-285 with maxRotDis = 0): its residual is the looked-up
// distance itself -- v - 0 and max(v, 0) are v bit for bit, the DT holds no negative value -- so the subtraction and the clamp are not issued.
// Bricked grids, x siblings less than 4 voxels apart (the deep expansions): the two x lookups of a (y, z) pair often lie in one 16-B x row
// of a brick, and one 16-B load then serves both (fewer cache-tag lookups than two dword gathers); the values are the same.

// Truncated search objective (opt-in, goicp_set_search_truncation; DtDesc::trunc = g > 0): every term of a bound is clamped at g AFTER its
// subtractions -- upper-bound term min(m, g)^2, lower-bound term min(max(m - delta, 0), g)^2 with m = max(DT - coeff |p|, 0) as ever.  Valid:
// rho_g(e) = min(e, g)^2 does not decrease in e >= 0, and max(m - delta, 0) is a lower bound of the residual of every pose of the cube, so
// rho_g of it is a lower bound of rho_g of that residual.  A grid clamped at g beforehand would give max(min(DT, g) - a, 0) instead: valid as
// well, but never larger and strictly smaller wherever DT > g and a > 0 (DT = 2 g, a = g: 0 against g) -- it forgets by how much a far point
// clears g, which is exactly what lets a cube full of outliers keep its floor n_out g^2 under a large radius.  So the clamp is on the term.
// min(max(x, 0), g) is ONE instruction, the median of (x, 0, g) for g >= 0, and takes the place of the untruncated form's max(x, 0): the
// truncated kernels issue no more vector instructions per term than the plain ones, except where the plain form had no clamp to replace
// (the pass without a rotation radius: one median per upper-bound term more).  g = +huge leaves every bit as it was.
__device__ __forceinline__ float trunc_clamp(float x, float g) { return __builtin_amdgcn_fmed3f(x, 0.f, g); }
__device__ __forceinline__ f2 trunc_clamp2(f2 x, float g) { return f2{trunc_clamp(x.x, g), trunc_clamp(x.y, g)}; }

// The float at byte offset `off` (bits 2-3) of a 16-B x row, picked with byte permutes: the selectors are per-lane VGPRs, where
// v_cndmask would hold four lane masks in SGPRs across the four loads (the kernel then spills SGPRs).  row_sel(off) = the two selectors.
struct RowSel { unsigned lo, hi; };
__device__ __forceinline__ RowSel row_sel(unsigned off)
{
	return RowSel{0x03020100u + (off & 4u) * 0x01010101u, 0x03020100u + ((off >> 1) & 4u) * 0x01010101u};
}
__device__ __forceinline__ float row_pick(const float4& r, RowSel s)
{
	const unsigned lo = __builtin_amdgcn_perm(__float_as_uint(r.y), __float_as_uint(r.x), s.lo);
	const unsigned hi = __builtin_amdgcn_perm(__float_as_uint(r.w), __float_as_uint(r.z), s.lo);
	return __uint_as_float(__builtin_amdgcn_perm(hi, lo, s.hi));
}
template <int LAYOUT, int NP, bool LAST_ZERO, bool TRUNC = false>
__device__ __forceinline__ void lean_points(const float4* __restrict__ src, int p0, int p1, const DtDesc& dt, const Rot9& R0, const SiblingSet& ts, float delta,
                                            const float (&coeff)[NP], f2 (&ub2)[NP][4], f2 (&lb2)[NP][4])
{
	const f2 delta2 = f2{delta, delta}, ndelta2 = f2{-delta, -delta};
	const bool merge_x = LAYOUT == 1 && (ts.tx1 - ts.tx0) * dt.scale_f < 4.f;      // uniform: one expansion per workgroup
	// one bound for the six margins: on the unchecked branch below every index is inside the grid, i.e. |F| < V, and eps(F) = c1 + c2 |F| grows with
	// |F|; a lane whose F lies outside takes the checked branch, which tests for itself (16 instead of 30 instructions for the test)
	const float eps_grid = __fmaf_rn((float)(dt.V + 1), dt.c2, dt.c1);
	for (int i = p0 + (int)threadIdx.x; i < p1; i += kBoundsThreads) {
		const float4 p = src[i];
		const float rx = R0.r[0] * p.x + R0.r[1] * p.y + R0.r[2] * p.z;
		const float ry = R0.r[3] * p.x + R0.r[4] * p.y + R0.r[5] * p.z;
		const float rz = R0.r[6] * p.x + R0.r[7] * p.y + R0.r[8] * p.z;
		const float qx[2] = {rx + ts.tx0, rx + ts.tx1}, qy[2] = {ry + ts.ty0, ry + ts.ty1}, qz[2] = {rz + ts.tz0, rz + ts.tz1};
		float F[6] = {__fmaf_rn(qx[0] - dt.xmin_f, dt.scale_f, 0.5f), __fmaf_rn(qx[1] - dt.xmin_f, dt.scale_f, 0.5f),
		              __fmaf_rn(qy[0] - dt.ymin_f, dt.scale_f, 0.5f), __fmaf_rn(qy[1] - dt.ymin_f, dt.scale_f, 0.5f),
		              __fmaf_rn(qz[0] - dt.zmin_f, dt.scale_f, 0.5f), __fmaf_rn(qz[1] - dt.zmin_f, dt.scale_f, 0.5f)};
		float worst = INFINITY;
#pragma unroll
		for (int k = 0; k < 6; k++) worst = fminf(worst, fabsf(F[k] - rintf(F[k])));
		int ix[2] = {(int)F[0], (int)F[1]}, iy[2] = {(int)F[2], (int)F[3]}, iz[2] = {(int)F[4], (int)F[5]};
		if (worst <= eps_grid) {
#pragma unroll
			for (int k = 0; k < 2; k++) {
				ix[k] = voxel_exact(qx[k], dt.xmin, dt.scale);
				iy[k] = voxel_exact(qy[k], dt.ymin, dt.scale);
				iz[k] = voxel_exact(qz[k], dt.zmin, dt.scale);
			}
		}
		const unsigned V = (unsigned)dt.V;
		const bool inside = (unsigned)ix[0] < V && (unsigned)ix[1] < V && (unsigned)iy[0] < V && (unsigned)iy[1] < V && (unsigned)iz[0] < V && (unsigned)iz[1] < V;
		float rho[NP];
#pragma unroll
		for (int q = 0; q < NP; q++) rho[q] = coeff[q] * p.w;
		if (__all(inside)) {
			unsigned fx[2], fy[2], fz[2];
#pragma unroll
			for (int k = 0; k < 2; k++) {
				// BYTE offsets (the lean variant only runs on grids of at most 256 MB: they fit 32 bits)
				if (LAYOUT == 0) { fx[k] = (unsigned)ix[k] << 2; fy[k] = __umul24((unsigned)iy[k], V) << 2; fz[k] = __umul24((unsigned)iz[k], V * V) << 2; }
				else {
					fx[k] = (((unsigned)ix[k] >> 2) << 8) | (brick_x((unsigned)ix[k]) << 2);
					fy[k] = (__umul24((unsigned)iy[k] >> 2, (unsigned)dt.VB) << 8) | (brick_y((unsigned)iy[k]) << 2);
					fz[k] = (__umul24((unsigned)iz[k] >> 2, (unsigned)(dt.VB * dt.VB)) << 8) | (brick_z((unsigned)iz[k]) << 2);
				}
			}
			const char* gb = reinterpret_cast<const char*>(dt.grid);
			unsigned yz[4];
#pragma unroll
			for (int k = 0; k < 4; k++) yz[k] = fy[k & 1] + fz[k >> 1];
			f2 vv[4];
			if (merge_x) {
				// one 16-B load of the x row holding ix[0] per (y, z) pair; ix[1] comes from the same row unless it lies in the next one
				// (fx[k] = brick << 8 | (ix[k] & 3) << 2: same row <=> equal above bit 3), and only those lanes make a second dword load
				const bool split = (fx[0] ^ fx[1]) >= 16u;
				const RowSel s0 = row_sel(fx[0]), s1 = row_sel(fx[1]);
				float4 row[4];
				float v1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
				for (int k = 0; k < 4; k++) row[k] = *reinterpret_cast<const float4*>(gb + ((fx[0] & ~15u) + yz[k]));
				if (split) {
#pragma unroll
					for (int k = 0; k < 4; k++) v1[k] = *reinterpret_cast<const float*>(gb + (fx[1] + yz[k]));
				}
#pragma unroll
				for (int k = 0; k < 4; k++) vv[k] = f2{row_pick(row[k], s0), split ? v1[k] : row_pick(row[k], s1)};
			} else {
#pragma unroll
				for (int k = 0; k < 4; k++) vv[k] = f2{*reinterpret_cast<const float*>(gb + (fx[0] + yz[k])), *reinterpret_cast<const float*>(gb + (fx[1] + yz[k]))};
			}
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const f2 v = vv[k];
#pragma unroll
				for (int q = 0; q < NP; q++) {
					f2 vq = v, mm = v;
					if constexpr (TRUNC) {
						if (!(LAST_ZERO && q == NP - 1)) vq = v - f2{rho[q], rho[q]};
						mm = trunc_clamp2(vq, dt.trunc);                   // the pass without a radius too: vq = v >= 0 there, the median is min(v, g)
						ub2[q][k] = ub2[q][k] + mm * mm;
						const f2 dis = trunc_clamp2(vq + ndelta2, dt.trunc);
						lb2[q][k] = lb2[q][k] + dis * dis;
					} else {
					if (!(LAST_ZERO && q == NP - 1)) {
						vq = v - f2{rho[q], rho[q]};
						mm = __builtin_elementwise_max(vq, f2{0.f, 0.f});
					}
					ub2[q][k] = ub2[q][k] + mm * mm;
					// max(mm - delta, 0) == max(vq - delta, 0) bit for bit (delta >= 0: vq < 0 gives 0 either way, vq >= 0 is mm; x + (-d) is x - d)
					const f2 dis = __builtin_elementwise_max(vq + ndelta2, f2{0.f, 0.f});
					lb2[q][k] = lb2[q][k] + dis * dis;
					}
				}
			}
		} else {
#pragma unroll
			for (int q = 0; q < NP; q++) {
				float m[kGroup];
				sibling_residuals<LAYOUT>(dt, R0, ts, p, rho[q], m);
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const f2 mm = f2{m[2 * k], m[2 * k + 1]};
					if constexpr (TRUNC) {
						const f2 mu = trunc_clamp2(mm, dt.trunc), dis = trunc_clamp2(mm - delta2, dt.trunc);
						ub2[q][k] = ub2[q][k] + mu * mu;
						lb2[q][k] = lb2[q][k] + dis * dis;
					} else {
					ub2[q][k] = ub2[q][k] + mm * mm;
					const f2 dis = __builtin_elementwise_max(mm - delta2, f2{0.f, 0.f});
					lb2[q][k] = lb2[q][k] + dis * dis;
					}
				}
			}
		}
	}
}

// ------------------------------------------------------------------------------------------------
// Pair form of the lean loop: TWO expansions of one rotation over one point chunk (launch_bounds, bounds_order = 2).  The point load, R p
// and |p| are shared; everything else is per member and is lean_points<.., 1, ..>'s own expression, in its order, on its thread: the six
// indices, the exactness test, the inside test, the gathers (merged x rows per member), the packed sums -- so every bound keeps its bits.
// Both members' gathers are issued before either is consumed.  The loop has no checked form: a member some lane of which leaves the grid
// is given up and evaluated again by the plain path (bounds_work), which decides per wavefront and point exactly as it always did.
// ------------------------------------------------------------------------------------------------
struct LeanIdx { int ix[2], iy[2], iz[2]; };
__device__ __forceinline__ bool lean_index(const DtDesc& dt, float rx, float ry, float rz, const SiblingSet& ts, float eps_grid, LeanIdx& o)
{
	const float qx[2] = {rx + ts.tx0, rx + ts.tx1}, qy[2] = {ry + ts.ty0, ry + ts.ty1}, qz[2] = {rz + ts.tz0, rz + ts.tz1};
	float F[6] = {__fmaf_rn(qx[0] - dt.xmin_f, dt.scale_f, 0.5f), __fmaf_rn(qx[1] - dt.xmin_f, dt.scale_f, 0.5f),
	              __fmaf_rn(qy[0] - dt.ymin_f, dt.scale_f, 0.5f), __fmaf_rn(qy[1] - dt.ymin_f, dt.scale_f, 0.5f),
	              __fmaf_rn(qz[0] - dt.zmin_f, dt.scale_f, 0.5f), __fmaf_rn(qz[1] - dt.zmin_f, dt.scale_f, 0.5f)};
	float worst = INFINITY;
#pragma unroll
	for (int k = 0; k < 6; k++) worst = fminf(worst, fabsf(F[k] - rintf(F[k])));
	o.ix[0] = (int)F[0]; o.ix[1] = (int)F[1]; o.iy[0] = (int)F[2]; o.iy[1] = (int)F[3]; o.iz[0] = (int)F[4]; o.iz[1] = (int)F[5];
	if (worst <= eps_grid) {
#pragma unroll
		for (int k = 0; k < 2; k++) {
			o.ix[k] = voxel_exact(qx[k], dt.xmin, dt.scale);
			o.iy[k] = voxel_exact(qy[k], dt.ymin, dt.scale);
			o.iz[k] = voxel_exact(qz[k], dt.zmin, dt.scale);
		}
	}
	const unsigned V = (unsigned)dt.V;
	return (unsigned)o.ix[0] < V && (unsigned)o.ix[1] < V && (unsigned)o.iy[0] < V && (unsigned)o.iy[1] < V && (unsigned)o.iz[0] < V && (unsigned)o.iz[1] < V;
}
// the eight looked-up values of a member whose indices all lie inside the bricked grid, as four x-sibling pairs (lean_points' gathers)
__device__ __forceinline__ void lean_gather(const DtDesc& dt, const LeanIdx& I, bool merge_x, f2 (&vv)[4])
{
	unsigned fx[2], fy[2], fz[2];
#pragma unroll
	for (int k = 0; k < 2; k++) {
		fx[k] = (((unsigned)I.ix[k] >> 2) << 8) | (brick_x((unsigned)I.ix[k]) << 2);
		fy[k] = (__umul24((unsigned)I.iy[k] >> 2, (unsigned)dt.VB) << 8) | (brick_y((unsigned)I.iy[k]) << 2);
		fz[k] = (__umul24((unsigned)I.iz[k] >> 2, (unsigned)(dt.VB * dt.VB)) << 8) | (brick_z((unsigned)I.iz[k]) << 2);
	}
	const char* gb = reinterpret_cast<const char*>(dt.grid);
	unsigned yz[4];
#pragma unroll
	for (int k = 0; k < 4; k++) yz[k] = fy[k & 1] + fz[k >> 1];
	if (merge_x) {
		const bool split = (fx[0] ^ fx[1]) >= 16u;
		const RowSel s0 = row_sel(fx[0]), s1 = row_sel(fx[1]);
		float4 row[4];
		float v1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
		for (int k = 0; k < 4; k++) row[k] = *reinterpret_cast<const float4*>(gb + ((fx[0] & ~15u) + yz[k]));
		if (split) {
#pragma unroll
			for (int k = 0; k < 4; k++) v1[k] = *reinterpret_cast<const float*>(gb + (fx[1] + yz[k]));
		}
#pragma unroll
		for (int k = 0; k < 4; k++) vv[k] = f2{row_pick(row[k], s0), split ? v1[k] : row_pick(row[k], s1)};
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++) vv[k] = f2{*reinterpret_cast<const float*>(gb + (fx[0] + yz[k])), *reinterpret_cast<const float*>(gb + (fx[1] + yz[k]))};
	}
}
template <bool LAST_ZERO, bool TRUNC>
__device__ __forceinline__ void lean_accum(const f2 (&vv)[4], float rho, f2 ndelta2, float g, f2 (&ub2)[4], f2 (&lb2)[4])
{
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const f2 v = vv[k];
		f2 vq = v, mm = v;
		if constexpr (TRUNC) {
			if (!LAST_ZERO) vq = v - f2{rho, rho};
			mm = trunc_clamp2(vq, g);
			ub2[k] = ub2[k] + mm * mm;
			const f2 dis = trunc_clamp2(vq + ndelta2, g);
			lb2[k] = lb2[k] + dis * dis;
		} else {
			if (!LAST_ZERO) {
				vq = v - f2{rho, rho};
				mm = __builtin_elementwise_max(vq, f2{0.f, 0.f});
			}
			ub2[k] = ub2[k] + mm * mm;
			const f2 dis = __builtin_elementwise_max(vq + ndelta2, f2{0.f, 0.f});
			lb2[k] = lb2[k] + dis * dis;
		}
	}
}
struct PairMember { SiblingSet ts; float delta, coeff; };
// okA / okB (wavefront-uniform): cleared when some lane of the wavefront left the grid under that member; the member's sums are then
// unfinished and the caller evaluates it again on the plain path, which owns the checked form
template <bool LZ_A, bool LZ_B, bool TRUNC>
__device__ __forceinline__ void lean_points_pair(const float4* __restrict__ src, int p0, int p1, const DtDesc& dt, const Rot9& R0, const PairMember& A, const PairMember& Bm,
                                                 f2 (&ubA)[4], f2 (&lbA)[4], f2 (&ubB)[4], f2 (&lbB)[4], bool& okA, bool& okB)
{
	const f2 ndA2 = f2{-A.delta, -A.delta}, ndB2 = f2{-Bm.delta, -Bm.delta};
	const bool mxA = (A.ts.tx1 - A.ts.tx0) * dt.scale_f < 4.f, mxB = (Bm.ts.tx1 - Bm.ts.tx0) * dt.scale_f < 4.f;      // uniform
	const float eps_grid = __fmaf_rn((float)(dt.V + 1), dt.c2, dt.c1);
	for (int i = p0 + (int)threadIdx.x; i < p1; i += kBoundsThreads) {
		const float4 p = src[i];
		const float rx = R0.r[0] * p.x + R0.r[1] * p.y + R0.r[2] * p.z;
		const float ry = R0.r[3] * p.x + R0.r[4] * p.y + R0.r[5] * p.z;
		const float rz = R0.r[6] * p.x + R0.r[7] * p.y + R0.r[8] * p.z;
		LeanIdx IA, IB;
		okA = okA && __all(lean_index(dt, rx, ry, rz, A.ts, eps_grid, IA));
		okB = okB && __all(lean_index(dt, rx, ry, rz, Bm.ts, eps_grid, IB));
		f2 va[4], vb[4];
		if (okA) lean_gather(dt, IA, mxA, va);
		if (okB) lean_gather(dt, IB, mxB, vb);
		if (okA) lean_accum<LZ_A, TRUNC>(va, A.coeff * p.w, ndA2, dt.trunc, ubA, lbA);
		if (okB) lean_accum<LZ_B, TRUNC>(vb, Bm.coeff * p.w, ndB2, dt.trunc, ubB, lbB);
	}
}

// the sums of one (expansion, chunk) work item: wave64 reduce, then the 4 wavefronts through LDS, then the item's row of the scratch block (or,
// unsplit, the bounds themselves).  also >= 0: a second group whose expansion is the same bit for bit (bounds_pair_kernel) gets the same sums
__device__ __forceinline__ void bounds_item_store(const float (&ub)[kGroup], const float (&lb)[kGroup], int group, int chunk, int chunks, int B,
                                                  float* __restrict__ scratch, float* __restrict__ ub_out, float* __restrict__ lb_out, float (*red)[2 * kGroup],
                                                  int also = -1)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c0 = group * kGroup;
#pragma unroll
	for (int c = 0; c < kGroup; c++) {
		float u = wave_sum(ub[c]), l = wave_sum(lb[c]);
		if (lane == 0) { red[wave][c] = u; red[wave][kGroup + c] = l; }
	}
	__syncthreads();
	if (threadIdx.x < 2 * kGroup) {
		float s = red[0][threadIdx.x];
#pragma unroll
		for (int w = 1; w < kBoundsThreads / 64; w++) s += red[w][threadIdx.x];
		if (chunks == 1) {
			int c = threadIdx.x & (kGroup - 1);
			if (c0 + c < B) (threadIdx.x < kGroup ? ub_out : lb_out)[c0 + c] = s;
			if (also >= 0 && also * kGroup + c < B) (threadIdx.x < kGroup ? ub_out : lb_out)[also * kGroup + c] = s;
		} else {
			scratch[((size_t)group * chunks + chunk) * (2 * kGroup) + threadIdx.x] = s;
			if (also >= 0) scratch[((size_t)also * chunks + chunk) * (2 * kGroup) + threadIdx.x] = s;
		}
	}
}

// twin test of the device-resident searches (bnbqueue.hip): the two searches of a rotation child -- upper-bound pass (coeff 0) and
// lower-bound pass -- often list the SAME translation node in the same round (the root always, most depth-1 and depth-2 nodes of the
// upper-bound pass).  The gathers of such a pair are identical; the lower-bound pass's item then evaluates both, the other leaves.
struct TwinCtx { const QSearch* searches; const int* psearch; int* sh; };
// a round of at least min_groups expansions walks its items in footprint order (launch_queue_sort below)
constexpr int kSortBins = 1 << 15;                // Morton cells, 5 bits per axis
__device__ __forceinline__ bool qsort_on(const QSort& qs, int ngroups) { return qs.order != nullptr && ngroups >= qs.min_groups; }

// work item `work` of `total` = groups*chunks: one (cube group, point chunk) pair
template <int LAYOUT, bool LEAN, bool TRUNC = false>
__device__ __forceinline__ void bounds_work(
    int work, int total, const float4* __restrict__ src, int N, const DtDesc& dt, const Rot9* __restrict__ rots,
    const CubeRec* __restrict__ cubes, const ParentRec* __restrict__ parents, int B, int groups, int chunks, int chunk_pts,
    float* __restrict__ scratch, float* __restrict__ ub_out, float* __restrict__ lb_out, float (*red)[2 * kGroup],
    const unsigned* __restrict__ order = nullptr, const TwinCtx tw = TwinCtx{nullptr, nullptr, nullptr})
{
	// XCD-aware tiling (speed only): blocks b and b+8 share an XCD (round-robin dispatch).  XCD x owns
	// the point chunks [x*cpx, (x+1)*cpx) -- a compact spatial patch of the k-d-ordered cloud -- and
	// walks the cube groups in order, so at any time one L2 serves gathers into the DT neighbourhood
	// of ONE patch under nearby translations (a few MB) instead of the whole surface band.
	int chunk, group;
	if (order) {
		// footprint-ordered items: XCD x walks the x-th eighth of the sorted list
		const int q = total >> 3, r = total & 7, x = work & 7, s = work >> 3;
		const unsigned t = order[(x <= r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + s];
		group = (int)(t / (unsigned)chunks);
		chunk = (int)t - group * chunks;
	} else if ((chunks & 7) == 0) {
		const int cpx = chunks >> 3, xcd = work & 7, slot = work >> 3;
		group = slot / cpx;
		chunk = xcd * cpx + (slot - group * cpx);
	} else {
		const int swz = xcd_remap(work, total);
		chunk = swz / groups; group = swz - chunk * groups;
	}
	const int c0 = group * kGroup;

	CubeRec cr[kGroup];
	load_group(cubes, parents, group, B, cr);
	bool uniform = true;
#pragma unroll
	for (int c = 0; c < kGroup; c++) uniform = uniform && (cr[c].rot == cr[0].rot);
	const Rot9 R0 = rots[cr[0].rot];
	// The 8 children of one BnB expansion share, per axis, only TWO translation values
	// (jly_goicp.cpp:267-273: corner + (j>>a & 1)*w + w/2), one rotation, one delta, one coeff.
	bool siblings = uniform && c0 + kGroup <= B;
#pragma unroll
	for (int c = 0; c < kGroup; c++)
		siblings = siblings && cr[c].tx == cr[c & 1].tx && cr[c].ty == cr[c & 2].ty && cr[c].tz == cr[c & 4].tz &&
		           cr[c].delta == cr[0].delta && cr[c].coeff == cr[0].coeff;

	float ub[kGroup], lb[kGroup];
#pragma unroll
	for (int c = 0; c < kGroup; c++) { ub[c] = 0.f; lb[c] = 0.f; }

	const int p0 = chunk * chunk_pts;
	const int p1 = p0 + chunk_pts < N ? p0 + chunk_pts : N;
	if (siblings) {
		// fast path: 6 voxel-index computations per point instead of 24; every per-point value is the
		// same float expression as in the generic path below, so the results are bit-identical
		const SiblingSet ts{cr[0].tx, cr[1].tx, cr[0].ty, cr[2].ty, cr[0].tz, cr[4].tz};
		const float delta = cr[0].delta, coeff = cr[0].coeff;
		// LEAN: lean_points (above).  Bunny microbench 1.837 -> 1.791 ms per launch, full registration 42.1 -> 40.6 ms; at 1 M points / 512^3
		// (HBM-bound) the same code is 13 % SLOWER (53.3 -> 60.5 ms), so the launch picks it by the size of the grid.
		if constexpr (LEAN && LAYOUT != 2) {
			// twin test (device-resident searches only): is this node also listed by the other search of the rotation child?
			int twin = -1;
			if (tw.searches) {
				const int ts_ = tw.searches[tw.psearch[group]].twin;
				if (ts_ >= 0) {
					const int tn = tw.searches[ts_].n_parents, toff = tw.searches[ts_].parent_off;
					if (tn > 0 && tw.searches[ts_].tile == 0) {
						if (threadIdx.x == 0) *tw.sh = -1;
						__syncthreads();
						for (int j = threadIdx.x; j < tn; j += kBoundsThreads) {       // tn <= kQueueMaxPop
							const ParentRec o = parents[toff + j], me = parents[group];
							if (o.x == me.x && o.y == me.y && o.z == me.z && o.w == me.w && o.rot == me.rot && (o.coeff == 0.f) != (me.coeff == 0.f)) *tw.sh = toff + j;
						}
						__syncthreads();
						twin = *tw.sh;
					}
				}
			}
			if (twin >= 0 && coeff == 0.f) return;              // the lower-bound pass's item evaluates this expansion for both
			if (twin >= 0) {
				f2 ub2[2][4], lb2[2][4];
#pragma unroll
				for (int q = 0; q < 2; q++)
#pragma unroll
					for (int k = 0; k < 4; k++) { ub2[q][k] = f2{0.f, 0.f}; lb2[q][k] = f2{0.f, 0.f}; }
				const float co[2] = {coeff, 0.f};
				lean_points<LAYOUT, 2, true, TRUNC>(src, p0, p1, dt, R0, ts, delta, co, ub2, lb2);
#pragma unroll
				for (int k = 0; k < 4; k++) { ub[2 * k] = ub2[1][k].x; ub[2 * k + 1] = ub2[1][k].y; lb[2 * k] = lb2[1][k].x; lb[2 * k + 1] = lb2[1][k].y; }
				bounds_item_store(ub, lb, twin, chunk, chunks, B, scratch, ub_out, lb_out, red);
				__syncthreads();                                  // `red` is reused for the item's own sums
#pragma unroll
				for (int k = 0; k < 4; k++) { ub[2 * k] = ub2[0][k].x; ub[2 * k + 1] = ub2[0][k].y; lb[2 * k] = lb2[0][k].x; lb[2 * k + 1] = lb2[0][k].y; }
			} else {
				f2 ub2[1][4], lb2[1][4];
#pragma unroll
				for (int k = 0; k < 4; k++) { ub2[0][k] = f2{0.f, 0.f}; lb2[0][k] = f2{0.f, 0.f}; }
				const float co[1] = {coeff};
				if (coeff == 0.f) lean_points<LAYOUT, 1, true, TRUNC>(src, p0, p1, dt, R0, ts, delta, co, ub2, lb2);       // block-uniform: one expansion per workgroup
				else lean_points<LAYOUT, 1, false, TRUNC>(src, p0, p1, dt, R0, ts, delta, co, ub2, lb2);
#pragma unroll
				for (int k = 0; k < 4; k++) { ub[2 * k] = ub2[0][k].x; ub[2 * k + 1] = ub2[0][k].y; lb[2 * k] = lb2[0][k].x; lb[2 * k + 1] = lb2[0][k].y; }
			}
		}
		else
		for (int i = p0 + (int)threadIdx.x; i < p1; i += kBoundsThreads) {
			const float4 p = src[i];
			float m[kGroup];
			sibling_residuals<LAYOUT>(dt, R0, ts, p, coeff * p.w, m);
#pragma unroll
			for (int c = 0; c < kGroup; c++) {
				if constexpr (TRUNC) {
					const float mu = trunc_clamp(m[c], dt.trunc), dis = trunc_clamp(m[c] - delta, dt.trunc);
					ub[c] += mu * mu;
					lb[c] += dis * dis;
				} else {
				ub[c] += m[c] * m[c];
				const float dis = fmaxf(m[c] - delta, 0.f);
				lb[c] += dis * dis;
				}
			}
		}
	} else
	for (int i = p0 + (int)threadIdx.x; i < p1; i += kBoundsThreads) {
		const float4 p = src[i];
		// p~ = R p (jly_goicp.cpp:470-476), left-to-right float sums
		float rx = R0.r[0] * p.x + R0.r[1] * p.y + R0.r[2] * p.z;
		float ry = R0.r[3] * p.x + R0.r[4] * p.y + R0.r[5] * p.z;
		float rz = R0.r[6] * p.x + R0.r[7] * p.y + R0.r[8] * p.z;
#pragma unroll
		for (int c = 0; c < kGroup; c++) {
			if (!uniform) {   // wave-uniform branch; generic batches only
				const Rot9 R = rots[cr[c].rot];
				rx = R.r[0] * p.x + R.r[1] * p.y + R.r[2] * p.z;
				ry = R.r[3] * p.x + R.r[4] * p.y + R.r[5] * p.z;
				rz = R.r[6] * p.x + R.r[7] * p.y + R.r[8] * p.z;
			}
			float m = dt_distance<LAYOUT>(dt, rx + cr[c].tx, ry + cr[c].ty, rz + cr[c].tz);
			m = m - cr[c].coeff * p.w;          // rotation uncertainty radius (jly_goicp.cpp:284-285, :159)
			if (m < 0.f) m = 0.f;
			if constexpr (TRUNC) {
				const float mu = trunc_clamp(m, dt.trunc), dis = trunc_clamp(m - cr[c].delta, dt.trunc);
				ub[c] += mu * mu;
				lb[c] += dis * dis;
			} else {
			ub[c] += m * m;                      // :302-306
			const float dis = fmaxf(m - cr[c].delta, 0.f);   // :312-314 (adding 0 when dis <= 0 is the same sum)
			lb[c] += dis * dis;
			}
		}
	}

	bounds_item_store(ub, lb, group, chunk, chunks, B, scratch, ub_out, lb_out, red);
}

// ------------------------------------------------------------------------------------------------
// LDS-staged DT tiles (north_star (a)): the bound evaluation for the DEEP expansions of one inner search.
//
// Late in a search the nodes an inner BnB expands are neighbours: the same rotation, translations a few voxels apart.
// For a small patch of the cloud (64 consecutive points of the k-d order) ALL their lookups -- 64 points x 8 siblings x
// up to 64 expansions = 32 768 -- then fall into one box of a few thousand voxels.  That box is copied from the bricked
// grid into LDS once (a few hundred 128-byte lines, coalesced) and the lookups become ds_read_b32.
//
// Mapping: a workgroup = 4 wavefronts = one (search, point chunk); a LANE = one expansion of the search (its two sibling
// translations per axis, delta, coeff live in registers); the 64 points of a sub-patch are dealt 16 to each wavefront and
// broadcast from LDS (rotated once per sub-patch).  No cross-lane reduction at all: a lane owns the 16 sums of its
// expansion over all the points its wavefront sees; the four wavefronts' sums are added in fixed order at the end.
// Every per-point value is the same float expression as in bounds_work (voxel_fast / voxel_exact, the same clamp and
// subtraction order); lookups that fall outside the staged box (or outside the grid) take dt_distance from global memory.
// ------------------------------------------------------------------------------------------------
#ifndef GOICP_TILE_FLOATS
#define GOICP_TILE_FLOATS 8192
#endif
constexpr int kTileFloats = GOICP_TILE_FLOATS;    // 32 KB: up to 128 bricks of 4x4x4 voxels
constexpr int kTilePatch = 64;                    // points per staged box
// split of the cloud for `nseg` tile segments on a grid of `grid` workgroups: as many chunks (multiples of the 64-point
// sub-patch) as it takes to give every workgroup an item, at most one sub-patch per chunk
__host__ __device__ inline void tile_shape(int nseg, int N, int grid, int* chunks, int* chunk_pts)
{
	const int patches = (N + kTilePatch - 1) / kTilePatch;
	int c = nseg > 0 ? (grid + nseg - 1) / nseg : 1;
	if (c < 1) c = 1;
	if (c > patches) c = patches;
	int cp = (patches + c - 1) / c * kTilePatch;
	c = (N + cp - 1) / cp;
	*chunks = c; *chunk_pts = cp;
}

// Round 3: the staged box is kept in LDS as a plain [z][y][x] array (brick-aligned origin and dimensions, so that it is
// still filled brick by brick with coalesced 16-byte loads), and a sub-patch whose box lies wholly inside the grid -- the
// usual case: the grid is the target's bounding cube expanded twice -- takes a path with NO per-lookup checks at all: the
// box contains, by construction, every voxel any lane can index for any of the 64 points, so a lookup is three
// multiply-adds, one three-operand add per child and a ds_read_b32; the eight children are accumulated as four pairs
// (x-siblings) in packed fp32 (v_pk_add / v_pk_mul -- same per-element operations and order as the scalar code:
// bit-identical).  Round 2's form computed brick offsets with a bounds check per axis and child (42 + 16 of its ~180
// vector instructions per point and lane, plus the branches around eight inlined global fallbacks).
__device__ __forceinline__ int add3(int a, int b, int c)
{
	int r;
	__asm__("v_add3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
	return r;
}

template <bool QUEUED, bool TRUNC = false>
__global__ __launch_bounds__(256) void bounds_tile_kernel(const float4* __restrict__ src, int N, DtDesc dt, const Rot9* __restrict__ rots,
                                                          const ParentRec* __restrict__ parents, const TileSeg* __restrict__ segs, int nseg_host, int chunks_host,
                                                          int chunk_pts_host, const int* __restrict__ d_nseg, int* __restrict__ d_chunks,
                                                          float* __restrict__ scratch, float* __restrict__ ub_out, float* __restrict__ lb_out,
                                                          unsigned* __restrict__ stats)
{
	__shared__ float tile[kTileFloats];
	__shared__ float4 rp[kTilePatch];             // R p of the sub-patch, w = |p|
	static_assert(4 * 64 * 2 * kGroup <= kTileFloats, "the wavefront sums reuse the tile");
	float (*wacc)[64][2 * kGroup] = reinterpret_cast<float (*)[64][2 * kGroup]>(tile);   // after the last sub-patch
	__shared__ float tr[6];                       // translation range of the search's siblings: min xyz, max xyz
	__shared__ int box[8];                        // voxel origin x0 y0 z0, voxel dims DX DY DZ (multiples of 4), staged, wholly inside the grid
	int nseg = nseg_host, chunks = chunks_host, chunk_pts = chunk_pts_host;
	if (QUEUED) {
		// the number of segments is known to the device only (bnb_queue_kernel counted them): the split of the cloud follows from it
		nseg = *d_nseg;
		if (nseg <= 0) return;
		tile_shape(nseg, N, (int)gridDim.x, &chunks, &chunk_pts);
		if (blockIdx.x == 0 && threadIdx.x == 0) *d_chunks = chunks;      // the next round's digest adds the chunk partials up
	}
	for (int item = blockIdx.x; item < nseg * chunks; item += QUEUED ? (int)gridDim.x : nseg * chunks) {
	const int seg = item / chunks, chunk = item - seg * chunks;
	const TileSeg sg = segs[seg];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	// A segment of n <= 32 expansions does not fill a wavefront with one expansion per lane: the lanes are dealt P = 2^ceil(log2 n)
	// expansions x L = 64 / P point subsets instead (lane = sub * P + e; lane group `sub` takes every L-th point of the wavefront's
	// share), and the L partial sums of an expansion are added at the end (xor shuffles, fixed order) -- at least half of the
	// lanes work for any n.
	int P = 1;
	while (P < sg.n) P <<= 1;
	const int L = 64 / P, e_lane = lane & (P - 1), sub = lane / P;
	const bool live = e_lane < sg.n;
	// this lane's expansion: corner + (bit)*w' + w'/2 per axis (load_group's float operations)
	const ParentRec pr = parents[sg.off + (live ? e_lane : 0)];
	const float w = pr.w / 2;
	const float delta = (float)(1.732050808 / 2.0 * (double)w);
	const SiblingSet ts{pr.x + w / 2, pr.x + w + w / 2, pr.y + w / 2, pr.y + w + w / 2, pr.z + w / 2, pr.z + w + w / 2};
	const float coeff = pr.coeff;
	const Rot9 R0 = rots[sg.rot];
	__syncthreads();                              // (queued form: the previous item's sums have been read out of the tile)
	if (wave == 0) {
		float mn[3] = {ts.tx0, ts.ty0, ts.tz0}, mx[3] = {ts.tx1, ts.ty1, ts.tz1};
#pragma unroll
		for (int k = 0; k < 3; k++) {
			if (!live) { mn[k] = INFINITY; mx[k] = -INFINITY; }
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o, 64)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o, 64)); }
			if (lane == 0) { tr[k] = mn[k]; tr[3 + k] = mx[k]; }
		}
	}
	f2 ub2[4], lb2[4];
#pragma unroll
	for (int k = 0; k < 4; k++) { ub2[k] = f2{0.f, 0.f}; lb2[k] = f2{0.f, 0.f}; }
	const f2 delta2 = f2{delta, delta}, ndelta2 = f2{-delta, -delta};
	const int p0 = chunk * chunk_pts, p1 = p0 + chunk_pts < N ? p0 + chunk_pts : N;
	__syncthreads();
	for (int s0 = p0; s0 < p1; s0 += kTilePatch) {
		// ---- the sub-patch: rotate, find the brick box of everything it can look up, stage it ----
		const int np = p1 - s0 < kTilePatch ? p1 - s0 : kTilePatch;
		if (threadIdx.x < kTilePatch) {
			int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
			if ((int)threadIdx.x < np) {
				const float4 p = src[s0 + threadIdx.x];
				const float rx = R0.r[0] * p.x + R0.r[1] * p.y + R0.r[2] * p.z;
				const float ry = R0.r[3] * p.x + R0.r[4] * p.y + R0.r[5] * p.z;
				const float rz = R0.r[6] * p.x + R0.r[7] * p.y + R0.r[8] * p.z;
				rp[threadIdx.x] = make_float4(rx, ry, rz, p.w);
				const float r3[3] = {rx, ry, rz}, m3[3] = {dt.xmin_f, dt.ymin_f, dt.zmin_f};
#pragma unroll
				for (int k = 0; k < 3; k++) {      // a voxel of margin each way: the box only has to CONTAIN the exact indices
					lo[k] = (int)floorf(((r3[k] + tr[k]) - m3[k]) * dt.scale_f + 0.5f) - 1;
					hi[k] = (int)floorf(((r3[k] + tr[3 + k]) - m3[k]) * dt.scale_f + 0.5f) + 1;
				}
			}
#pragma unroll
			for (int k = 0; k < 3; k++) {
#pragma unroll
				for (int o = 32; o > 0; o >>= 1) { lo[k] = min(lo[k], __shfl_xor(lo[k], o, 64)); hi[k] = max(hi[k], __shfl_xor(hi[k], o, 64)); }
			}
			if (threadIdx.x == 0) {
				// the box in LDS: x brick-aligned (it is filled with 16-byte pieces of brick rows), y and z exact
				bool inside = true;
#pragma unroll
				for (int k = 0; k < 3; k++) inside = inside && lo[k] >= 0 && hi[k] <= dt.V - 1;
				const int x0 = lo[0] & ~3, DX = ((hi[0] | 3) + 1) - x0, DY = hi[1] - lo[1] + 1, DZ = hi[2] - lo[2] + 1;
				const bool ok = inside && (long long)DX * DY * DZ <= kTileFloats;
				box[0] = x0; box[1] = lo[1]; box[2] = lo[2]; box[3] = DX; box[4] = DY; box[5] = DZ;
				box[6] = ok ? 1 : 0; box[7] = ok ? 1 : 0;
				if (stats) atomicAdd(&stats[ok ? 0 : 1], 1u);
			}
		}
		__syncthreads();
		const int x0 = box[0], y0 = box[1], z0 = box[2], DX = box[3], DY = box[4], DZ = box[5];
		const bool fast = box[7] != 0;
		if (fast) {
			// every brick the box touches is read whole (16 consecutive lanes = one 256-byte brick: coalesced), the pieces inside
			// the box are kept
			const int bx0 = x0 >> 2, by0 = y0 >> 2, bz0 = z0 >> 2;
			const int nbx = DX >> 2, nby = ((y0 + DY - 1) >> 2) - by0 + 1, nbz = ((z0 + DZ - 1) >> 2) - bz0 + 1;
			const int n4 = nbx * nby * nbz * 16;
			// brick number -> (bx, by, bz) without integer division (two of them cost ~50 instructions per 16-byte piece): the quotient of b + 0.5 by
			// a count n < 64 in float is exact for b < 2^21 -- it is at least 0.5 / n away from an integer, the rounding errors stay below that
			const float rnbx = 1.0f / (float)nbx, rnby = 1.0f / (float)nby;
			for (int idx = threadIdx.x; idx < n4; idx += 256) {
				const int b = idx >> 4, part = idx & 15;
				const int t2 = (int)(((float)b + 0.5f) * rnbx), bx = b - t2 * nbx;
				const int bz = (int)(((float)t2 + 0.5f) * rnby), by = t2 - bz * nby;
				const int y = (by0 + by) * 4 + (part & 3) - y0, z = (bz0 + bz) * 4 + (part >> 2) - z0;       // piece = x row (brick_y | brick_z) >> 2
				const size_t gb = ((size_t)(bz0 + bz) * dt.VB + (by0 + by)) * dt.VB + (bx0 + bx);
				const float4 v = reinterpret_cast<const float4*>(dt.grid)[gb * 16 + part];
				if ((unsigned)y < (unsigned)DY && (unsigned)z < (unsigned)DZ) *reinterpret_cast<float4*>(&tile[(z * DY + y) * DX + bx * 4]) = v;
			}
		}
		__syncthreads();
		// ---- every wavefront: its 16 points x this lane's 8 siblings ----
		if (live) {
			if (fast) {
				// byte address in the tile = 4 (ix - x0) + 4 DX (iy - y0) + 4 DX DY (iz - z0)
				const int sy = 4 * DX, sz = 4 * DX * DY;
				const int cxyz = -4 * x0 - sy * y0 - sz * z0;
				const float eps_box = __fmaf_rn((float)dt.V, dt.c2, dt.c1);
				const char* tb = reinterpret_cast<const char*>(tile);
				// A segment is one search: all its lanes make the same pass.  In the upper-bound pass (coeff == 0, jly_goicp.cpp:284-285 with
				// maxRotDis = 0) the residual is the looked-up distance itself: v - 0 and max(v, 0) are v bit for bit (the DT holds no negative
				// value), so that pass runs a loop without the subtraction and the clamp (12 of ~90 vector instructions per point).
				auto patch_points = [&](auto ub_pass) {
				constexpr bool UB_PASS = decltype(ub_pass)::value;
				for (int j = wave + 4 * sub; j < np; j += 4 * L) {
					const float4 q = rp[j];                               // one address per lane group: a broadcast read
					const float qx[2] = {q.x + ts.tx0, q.x + ts.tx1}, qy[2] = {q.y + ts.ty0, q.y + ts.ty1}, qz[2] = {q.z + ts.tz0, q.z + ts.tz1};
					// six voxel indices: F = (q - min) * scale + 0.5 in float; the float index is provably the reference's unless F is
					// within eps(F) = c1 + c2 |F| of an integer (voxel_fast) -- ONE test on the smallest margin of the six
					float F[6] = {__fmaf_rn(qx[0] - dt.xmin_f, dt.scale_f, 0.5f), __fmaf_rn(qx[1] - dt.xmin_f, dt.scale_f, 0.5f),
					              __fmaf_rn(qy[0] - dt.ymin_f, dt.scale_f, 0.5f), __fmaf_rn(qy[1] - dt.ymin_f, dt.scale_f, 0.5f),
					              __fmaf_rn(qz[0] - dt.zmin_f, dt.scale_f, 0.5f), __fmaf_rn(qz[1] - dt.zmin_f, dt.scale_f, 0.5f)};
					// (the box lies inside the grid, so 0 <= F < V on this path: ONE bound eps(V) >= eps(F) serves all six -- a few more lanes take the
					// exact branch, none takes a wrong index; 16 instead of 29 instructions for the test)
					float margin[6];
#pragma unroll
					for (int k = 0; k < 6; k++) margin[k] = fabsf(F[k] - rintf(F[k]));
					const float worst = fminf(fminf(fminf(margin[0], margin[1]), fminf(margin[2], margin[3])), fminf(margin[4], margin[5]));
					int ix[2] = {(int)F[0], (int)F[1]}, iy[2] = {(int)F[2], (int)F[3]}, iz[2] = {(int)F[4], (int)F[5]};
					if (worst <= eps_box) {
#pragma unroll
						for (int k = 0; k < 2; k++) {
							ix[k] = voxel_exact(qx[k], dt.xmin, dt.scale);
							iy[k] = voxel_exact(qy[k], dt.ymin, dt.scale);
							iz[k] = voxel_exact(qz[k], dt.zmin, dt.scale);
						}
					}
					// the three origin terms ride on the x part; one three-operand add per child (the compiler would share y + z sums: 12 adds for 8)
					const int ax[2] = {4 * ix[0] + cxyz, 4 * ix[1] + cxyz};
					const int ay[2] = {__mul24(iy[0], sy), __mul24(iy[1], sy)};
					const int az[2] = {__mul24(iz[0], sz), __mul24(iz[1], sz)};
					const float rho = coeff * q.w;
					const f2 rho2 = f2{rho, rho};
#pragma unroll
					for (int k = 0; k < 4; k++) {                         // pair k: children 2k (x0) and 2k + 1 (x1) of y[(k & 1)], z[(k >> 1)]
						f2 v = f2{*reinterpret_cast<const float*>(tb + add3(ax[0], ay[k & 1], az[k >> 1])), *reinterpret_cast<const float*>(tb + add3(ax[1], ay[k & 1], az[k >> 1]))};
						f2 m = v;
						if constexpr (TRUNC) {
							if constexpr (!UB_PASS) v = v - rho2;
							m = trunc_clamp2(v, dt.trunc);                        // (the upper-bound pass too: v >= 0 there, the median is min(v, g))
							ub2[k] = ub2[k] + m * m;
							const f2 dis = trunc_clamp2(v + ndelta2, dt.trunc);
							lb2[k] = lb2[k] + dis * dis;
						} else {
						if constexpr (!UB_PASS) {
							v = v - rho2;
							m = __builtin_elementwise_max(v, f2{0.f, 0.f});
						}
						ub2[k] = ub2[k] + m * m;
						// max(m - delta, 0) == max(v - delta, 0) bit for bit (delta >= 0: v < 0 gives 0 either way, v >= 0 is m), and the
						// subtraction no longer waits for the clamp (a packed subtract of the packed difference)
						const f2 dis = __builtin_elementwise_max(v + ndelta2, f2{0.f, 0.f});      // x + (-d) is x - d bit for bit
						lb2[k] = lb2[k] + dis * dis;
						}
					}
				}
				};
				if (__builtin_amdgcn_readfirstlane(__float_as_int(coeff)) == 0 && coeff == 0.f) patch_points(std::true_type{});
				else patch_points(std::false_type{});
			} else {
				// the box is too large for the tile, or reaches over the edge of the grid: the direct kernel's sibling path (eight
				// gathers in flight per point, out-of-grid extension included) -- same per-point expressions
				for (int j = wave + 4 * sub; j < np; j += 4 * L) {
					const float4 q = rp[j];
					float m[kGroup];
					sibling_residuals_rotated<1>(dt, q, ts, coeff * q.w, m);
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const f2 m2 = f2{m[2 * k], m[2 * k + 1]};
						if constexpr (TRUNC) {
							const f2 mu = trunc_clamp2(m2, dt.trunc), dis = trunc_clamp2(m2 - delta2, dt.trunc);
							ub2[k] = ub2[k] + mu * mu;
							lb2[k] = lb2[k] + dis * dis;
						} else {
						ub2[k] = ub2[k] + m2 * m2;
						const f2 dis = __builtin_elementwise_max(m2 - delta2, f2{0.f, 0.f});
						lb2[k] = lb2[k] + dis * dis;
						}
					}
				}
			}
		}
		__syncthreads();                                                  // the box is restaged by the next sub-patch
	}
	// ---- the lane groups' partial sums of an expansion (L > 1), then the four wavefronts' sums, in fixed order ----
	for (int off = P; off < 64; off <<= 1) {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			ub2[k].x += __shfl_xor(ub2[k].x, off, 64); ub2[k].y += __shfl_xor(ub2[k].y, off, 64);
			lb2[k].x += __shfl_xor(lb2[k].x, off, 64); lb2[k].y += __shfl_xor(lb2[k].y, off, 64);
		}
	}
#pragma unroll
	for (int k = 0; k < 4; k++) {
		wacc[wave][lane][2 * k] = ub2[k].x; wacc[wave][lane][2 * k + 1] = ub2[k].y;
		wacc[wave][lane][kGroup + 2 * k] = lb2[k].x; wacc[wave][lane][kGroup + 2 * k + 1] = lb2[k].y;
	}
	__syncthreads();
	for (int idx = threadIdx.x; idx < sg.n * 2 * kGroup; idx += 256) {
		const int e = idx >> 4, k = idx & 15;
		const float s = ((wacc[0][e][k] + wacc[1][e][k]) + wacc[2][e][k]) + wacc[3][e][k];
		const int group = sg.off + e;
		if (chunks == 1) (k < kGroup ? ub_out : lb_out)[group * kGroup + (k & (kGroup - 1))] = s;
		else scratch[((size_t)group * chunks + chunk) * (2 * kGroup) + k] = s;
	}
	}
}

__global__ void bounds_finalize(const float* __restrict__ scratch, int B, int groups, int chunks, float* __restrict__ ub_out, float* __restrict__ lb_out,
                                const int* __restrict__ alias, const int* __restrict__ ctl);
// test / measurement entry: nseg searches of n <= 64 expansions each (segment i = parents[i*n .. i*n+n), rotation i)
hipError_t launch_bounds_tile(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const ParentRec* parents, const void* segs, int nseg, int n,
                              int chunks, float* scratch, float* ub, float* lb, unsigned* stats, hipStream_t stream)
{
	if (dt.layout != 1 || n < 1 || n > 64 || nseg < 1 || chunks < 1) return hipErrorInvalidValue;
	int cp = (N + chunks - 1) / chunks;
	cp = (cp + kTilePatch - 1) / kTilePatch * kTilePatch;
	hipLaunchKernelGGL((dt.trunc > 0.f ? bounds_tile_kernel<false, true> : bounds_tile_kernel<false>), dim3(nseg * chunks), dim3(256), 0, stream, src, N, dt, rots, parents,
	                   static_cast<const TileSeg*>(segs), nseg, chunks, cp, static_cast<const int*>(nullptr), static_cast<int*>(nullptr), scratch, ub, lb, stats);
	if (chunks > 1) {
		const int groups = nseg * n, t = groups * 2 * kGroup;
		hipLaunchKernelGGL(bounds_finalize, dim3((t + 255) / 256), dim3(256), 0, stream, scratch, groups * kGroup, groups, chunks, ub, lb, (const int*)nullptr, (const int*)nullptr);
	}
	return hipGetLastError();
}

// the lean sibling path pays while the grid is cache-resident (<= the 256 MB Infinity Cache), not when the launch is HBM-bound
static inline bool bounds_lean(const DtDesc& dt) { return (size_t)dt.V * dt.V * dt.V * sizeof(float) <= ((size_t)256 << 20); }
bool bounds_uses_lean(const DtDesc& dt) { return dt.layout == 1 && bounds_lean(dt); }
constexpr int kTileQueueGrid = 256 * (160 * 1024 / (kTileFloats * 4 + 2048));   // as many workgroups per CU as their LDS allows (32 KB tiles: four)
int bounds_tile_queue_grid() { return kTileQueueGrid; }
size_t bounds_tile_queue_scratch_floats(int max_groups)
{
	// groups x chunks x 16 with chunks <= ceil(grid / segments) and groups <= 64 segments: at most 64 (grid + segments) rows
	return (size_t)64 * ((size_t)kTileQueueGrid + (size_t)max_groups) * 2 * kGroup;
}
hipError_t launch_bounds_tile_queue(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const QTile& tile, QCtl* ctl, int parity, hipStream_t stream)
{
	if (dt.layout != 1 || N <= 0) return hipErrorInvalidValue;
	hipLaunchKernelGGL((dt.trunc > 0.f ? bounds_tile_kernel<true, true> : bounds_tile_kernel<true>), dim3(kTileQueueGrid), dim3(256), 0, stream, src, N, dt, rots, tile.parents[parity], tile.segs[parity], 0, 1, 0,
	                   &ctl->n_tile_segs[parity], &ctl->tile_chunks, tile.scratch, tile.ub, tile.lb, static_cast<unsigned*>(nullptr));
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Grouping of an UNRELATED cube batch (the operator API's arbitrary batches; SURVEY 8(d)'s microbench): cubes are bucketed by
// (rotation, pass, 12-bit Morton cell of the translation) with a counting sort, evaluated in that order -- a workgroup's eight
// cubes then share their rotation and lie in one translation cell, and neighbouring workgroups gather from neighbouring DT
// lines -- and the bounds are written back to the caller's order.  Bounds are per cube, so the order changes no bit of them
// (tools/generic_probe.py: 3.75 -> 2.2 ms per 65 536 unrelated cubes on the bunny).  The search never needs this: its expansions
// arrive grouped by search, eight siblings at a time.
// ------------------------------------------------------------------------------------------------
constexpr int kGroupCellBits = 4;                  // per axis: 16 x 16 x 16 translation cells over [-0.5, 0.5]^3 (clamped outside)
__device__ __forceinline__ unsigned cube_bucket(const CubeRec& c, int nrots)
{
	unsigned m = 0;
	const float t[3] = {c.tx, c.ty, c.tz};
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const int q = min(max((int)((t[k] + 0.5f) * (float)(1 << kGroupCellBits)), 0), (1 << kGroupCellBits) - 1);
#pragma unroll
		for (int b = 0; b < kGroupCellBits; b++) m |= (unsigned)((q >> b) & 1) << (3 * b + k);
	}
	const unsigned rot = (unsigned)min(max(c.rot, 0), nrots - 1);
	return ((rot * 2u + (c.coeff > 0.f ? 1u : 0u)) << (3 * kGroupCellBits)) | m;
}
__global__ void cube_hist_kernel(const CubeRec* __restrict__ cubes, int B, int nrots, unsigned* __restrict__ hist)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < B) atomicAdd(&hist[cube_bucket(cubes[i], nrots)], 1u);
}
// exclusive scan of nbins counters, one workgroup of 1024 threads (nbins <= 1024 * 64)
__global__ __launch_bounds__(1024) void cube_scan_kernel(unsigned* __restrict__ hist, int nbins)
{
	__shared__ unsigned wtot[16];
	const int per = (nbins + 1023) / 1024, b0 = threadIdx.x * per;
	unsigned local = 0;
	for (int k = 0; k < per; k++) if (b0 + k < nbins) local += hist[b0 + k];
	unsigned incl = local;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if ((int)(threadIdx.x & 63) >= o) incl += v; }
	if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
	__syncthreads();
	unsigned before = 0;
	for (int w = 0; w < (int)(threadIdx.x >> 6); w++) before += wtot[w];
	unsigned run = before + incl - local;
	for (int k = 0; k < per; k++) if (b0 + k < nbins) { const unsigned c = hist[b0 + k]; hist[b0 + k] = run; run += c; }
}
__global__ void cube_scatter_kernel(const CubeRec* __restrict__ cubes, int B, int nrots, unsigned* __restrict__ offs, CubeRec* __restrict__ sorted, int* __restrict__ perm)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= B) return;
	const CubeRec c = cubes[i];
	const unsigned pos = atomicAdd(&offs[cube_bucket(c, nrots)], 1u);        // order inside a bucket is arbitrary: the bounds do not depend on it
	sorted[pos] = c;
	perm[pos] = i;
}
__global__ void cube_unpermute_kernel(const float* __restrict__ ub_s, const float* __restrict__ lb_s, const int* __restrict__ perm, int B, float* __restrict__ ub,
                                      float* __restrict__ lb)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= B) return;
	const int o = perm[i];
	ub[o] = ub_s[i]; lb[o] = lb_s[i];
}
size_t bounds_grouped_scratch_bytes(int B, int nrots)
{
	const size_t nbins = (size_t)nrots * 2 << (3 * kGroupCellBits);
	return sizeof(unsigned) * nbins + (sizeof(CubeRec) + sizeof(int) + 2 * sizeof(float)) * (size_t)B + 256;
}
hipError_t launch_bounds_grouped(const float4* src, int N, const DtDesc& dt, const Rot9* rots, int nrots, const CubeRec* cubes, int B, void* group_scratch,
                                 float* scratch, float* ub, float* lb, hipStream_t stream)
{
	if (B <= 0 || N <= 0) return hipSuccess;
	const int nbins = (nrots * 2) << (3 * kGroupCellBits);
	if (nrots < 1 || nbins > 1024 * 64) return hipErrorInvalidValue;
	char* p = static_cast<char*>(group_scratch);
	unsigned* hist = reinterpret_cast<unsigned*>(p); p += sizeof(unsigned) * (size_t)nbins;
	p = reinterpret_cast<char*>(((uintptr_t)p + 63) & ~(uintptr_t)63);
	CubeRec* sorted = reinterpret_cast<CubeRec*>(p); p += sizeof(CubeRec) * (size_t)B;
	int* perm = reinterpret_cast<int*>(p); p += sizeof(int) * (size_t)B;
	float* ub_s = reinterpret_cast<float*>(p); p += sizeof(float) * (size_t)B;
	float* lb_s = reinterpret_cast<float*>(p);
	hipError_t e = hipMemsetAsync(hist, 0, sizeof(unsigned) * (size_t)nbins, stream);
	if (e != hipSuccess) return e;
	const dim3 g((B + 255) / 256), b(256);
	hipLaunchKernelGGL(cube_hist_kernel, g, b, 0, stream, cubes, B, nrots, hist);
	hipLaunchKernelGGL(cube_scan_kernel, dim3(1), dim3(1024), 0, stream, hist, nbins);
	hipLaunchKernelGGL(cube_scatter_kernel, g, b, 0, stream, cubes, B, nrots, hist, sorted, perm);
	e = launch_bounds(src, N, dt, rots, sorted, nullptr, B, scratch, ub_s, lb_s, stream);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(cube_unpermute_kernel, g, b, 0, stream, ub_s, lb_s, perm, B, ub, lb);
	return hipGetLastError();
}

template <int LAYOUT, bool LEAN = false, bool TRUNC = false>
__global__ __launch_bounds__(kBoundsThreads) void bounds_kernel(
    const float4* __restrict__ src, int N, DtDesc dt, const Rot9* __restrict__ rots,
    const CubeRec* __restrict__ cubes, const ParentRec* __restrict__ parents, int B, int groups, int chunks, int chunk_pts,
    float* __restrict__ scratch, float* __restrict__ ub_out, float* __restrict__ lb_out)
{
	__shared__ float red[kBoundsThreads / 64][2 * kGroup];
	bounds_work<LAYOUT, LEAN, TRUNC>(blockIdx.x, gridDim.x, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub_out, lb_out, red);
}

// ------------------------------------------------------------------------------------------------
// Footprint order of a PLAIN bound launch (launch_bounds with a BoundsOrder; the engine passes one for cube batches handed in on the
// device).  Such a batch carries no rotation count and arrives in any translation order, so the pre-pass keys its G = ceil(B / 8) groups by
// the RUN of equal rotation they arrive in (a rotation that recurs later starts a new run) and, inside a run, by the Morton cell of the
// parent cube's centre in DT voxels: 5 bits per axis over the run's own extent, cells no smaller than cell_vox.  One workgroup per run:
// every workgroup finds the run starts for itself (each group's rotation against its predecessor's), then counting-sorts its run in LDS and
// writes its slice of order[] and, two neighbours of the order at a time, of the pair list (a leftover stays single).  More runs than max_runs
// (unrelated cubes): ctl = (0, 0), the launch walks the groups as they came.  The order inside a cell is whatever the atomics give: no bound
// depends on it, every group writes its own rows.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int group_rot(const CubeRec* __restrict__ cubes, int g) { return cubes[(size_t)g * kGroup].rot; }
__device__ __forceinline__ void group_centre(const CubeRec* __restrict__ cubes, int g, int B, float (&c)[3])
{
	const int i0 = g * kGroup, i1 = min(i0 + kGroup - 1, B - 1);
	const CubeRec a = cubes[i0], b = cubes[i1];                       // children 0 and 7 of an expansion: their mean is the parent's centre
	c[0] = 0.5f * (a.tx + b.tx); c[1] = 0.5f * (a.ty + b.ty); c[2] = 0.5f * (a.tz + b.tz);
}
// bounds_work's item mapping and its inverse: the new kernels pick (group, chunk) themselves and hand bounds_work the index that maps to it,
// so that bounds_work -- and with it every kernel that was there before -- stays as it was
__device__ __forceinline__ void bounds_item_of(int work, int total, int groups, int chunks, int& group, int& chunk)
{
	if ((chunks & 7) == 0) {
		const int cpx = chunks >> 3, xcd = work & 7, slot = work >> 3;
		group = slot / cpx;
		chunk = xcd * cpx + (slot - group * cpx);
	} else {
		const int swz = xcd_remap(work, total);
		chunk = swz / groups; group = swz - chunk * groups;
	}
}
__device__ __forceinline__ int bounds_work_of(int group, int chunk, int groups, int chunks)
{
	if ((chunks & 7) == 0) {
		const int cpx = chunks >> 3, xcd = chunk / cpx;
		return ((group * cpx + (chunk - xcd * cpx)) << 3) | xcd;
	}
	const int nb = groups * chunks, q = nb >> 3, r = nb & 7, swz = chunk * groups + group;
	int xcd, off;
	if (swz < r * (q + 1)) { xcd = swz / (q + 1); off = swz - xcd * (q + 1); }
	else { const int t = swz - r * (q + 1); xcd = r + t / q; off = t - (xcd - r) * q; }
	return (off << 3) | xcd;
}
// the 15-bit Morton cell of a centre: 5 bits per axis, cells of 1 / to_cell from the run's low corner
__device__ __forceinline__ unsigned order_key(const float (&c)[3], const float (&lo)[3], float to_cell)
{
	unsigned key = 0;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const unsigned v = (unsigned)min(max((int)((c[k] - lo[k]) * to_cell), 0), 31);
#pragma unroll
		for (int b = 0; b < 5; b++) key |= ((v >> b) & 1u) << (3 * b + k);
	}
	return key;
}
// the table key of a full group: its children 0 and 7 (what group_centre reads) as raw words, rotation and coefficient included
__device__ __forceinline__ unsigned alias_hash(const CubeRec& a, const CubeRec& b)
{
	const unsigned w[12] = {__float_as_uint(a.tx), __float_as_uint(a.ty), __float_as_uint(a.tz), __float_as_uint(a.delta), __float_as_uint(a.coeff), (unsigned)a.rot,
	                        __float_as_uint(b.tx), __float_as_uint(b.ty), __float_as_uint(b.tz), __float_as_uint(b.delta), __float_as_uint(b.coeff), (unsigned)b.rot};
	unsigned h = 0x9e3779b9u;
#pragma unroll
	for (int k = 0; k < 12; k++) { h = (h ^ w[k]) * 0x85ebca6bu; h ^= h >> 15; }
	return h;
}
// are the eight records of two full groups the same 48 words?  raw bits: -0 against +0, or one ulp anywhere, is another expansion
__device__ __forceinline__ bool same_records(const CubeRec* __restrict__ cubes, int ga, int gb)
{
	constexpr int nw = kGroup * (int)(sizeof(CubeRec) / sizeof(unsigned));
	const unsigned* a = reinterpret_cast<const unsigned*>(cubes + (size_t)ga * kGroup);
	const unsigned* b = reinterpret_cast<const unsigned*>(cubes + (size_t)gb * kGroup);
	unsigned d = 0u;
#pragma unroll
	for (int k = 0; k < nw; k++) d |= a[k] ^ b[k];
	return d == 0u;
}
// No step of the pre-pass waits on a chain of loads.  Run starts: thread t compares the rotation of groups t, t + 1024, ... with their
// predecessors' (independent loads, all in flight together); the at most 63 boundaries take a slot of an LDS list and are ranked there.  A
// thread keeps the centres and keys of its first kOrderHeld groups of the run in registers from the extent to the scatter (a longer run
// loads the rest again in each phase), and the scatter writes order[] and the pair list straight from the slot the counting sort hands out.
constexpr int kOrderHeld = 4;                        // runs of up to 4 096 groups; eight spill at the 128 VGPRs of a 1 024-thread workgroup
// The first wavefront of block 0 leaves the cuts of the pair launch's 8-chunk shape behind ctl[0..3] on both exits: lane x forms cut[x] from the
// plan the source cloud left (bounds_cut_of: one division, all nine side by side), the bound of a piece is enforced along the lanes
// (bounds_cut_cap's two passes), lanes 0 .. 8 store.  balanced = 0: the equal split.  Called by all 64 lanes of the wavefront.
__device__ __forceinline__ void bounds_cuts_store(const BoundsOrder& bo, int balanced, int items, int lane)
{
	const int x = min(lane, 8);
	int cut = balanced ? bounds_cut_of(bo.cost + kBoundsCost, x, items) : x * items;
	if (balanced) {
		const int cap = (int)(((long long)items * 5 + 3) / 4);
		for (int k = 1; k < 8; k++) { const int prev = __shfl(cut, k - 1, 64); if (lane == k) cut = min(cut, prev + cap); }
		for (int k = 7; k >= 1; k--) { const int next = __shfl(cut, k + 1, 64); if (lane == k) cut = max(cut, next - cap); }
	}
	if (lane <= 8) bo.ctl[kBoundsCut + lane] = cut;
}
__global__ __launch_bounds__(1024) void bounds_order_kernel(const CubeRec* __restrict__ cubes, int B, int G, DtDesc dt, BoundsOrder bo, int balanced)
{
	constexpr int per = kSortBins / 1024;            // 32 consecutive bins per thread, padded against the bank conflict (task_scan_kernel)
	constexpr int words = kSortBins + kSortBins / per;
	__shared__ __attribute__((aligned(16))) unsigned lds[words];
	__shared__ unsigned wtot[16];
	__shared__ int run_start[kBoundsOrderMaxRuns + 2];
	__shared__ int bound[kBoundsOrderMaxRuns];
	__shared__ int nbound;
	__shared__ float ext[16][6];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	static_assert(words % 4 == 0, "the counters are cleared four at a time");
	for (int i = tid; i < words / 4; i += 1024) reinterpret_cast<uint4*>(lds)[i] = make_uint4(0u, 0u, 0u, 0u);
	if (tid == 0) nbound = 0;
	__syncthreads();
	// the runs of equal rotation, in arrival order
	for (int base = 0; base < G; base += 8 * 1024) {
		int r[8], p[8];
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const int g = min(base + k * 1024 + tid, G - 1);
			r[k] = group_rot(cubes, g);
			p[k] = lane == 0 ? group_rot(cubes, g > 0 ? g - 1 : 0) : 0;   // a group's record is a cache line of its own: the other lanes take the predecessor from their neighbour
		}
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const int g = base + k * 1024 + tid, up = __shfl_up(r[k], 1, 64);
			if (lane) p[k] = up;
			if (g < G && r[k] != p[k]) { const int slot = atomicAdd(&nbound, 1); if (slot < kBoundsOrderMaxRuns) bound[slot] = g; }
		}
	}
	__syncthreads();
	const int nb = nbound, runs = nb + 1;
	if (runs > bo.max_runs) {
		if (blockIdx.x == 0 && tid == 0) {
			bo.ctl[0] = 0; bo.ctl[1] = 0; bo.ctl[2] = 0; bo.ctl[3] = 0; bo.ctl[kBoundsCopies] = 0; if (bo.host_note) *bo.host_note = ((long long)G << 1) | 1;
		}
		if (blockIdx.x == 0 && tid < 64) bounds_cuts_store(bo, balanced, (G + 1) >> 1, tid);
		return;
	}
	if (tid == 0) { run_start[0] = 0; run_start[runs] = G; }
	if (tid < nb) {                                      // nb < max_runs <= kBoundsOrderMaxRuns: every boundary has its slot
		const int b = bound[tid];
		int rank = 1;
		for (int q = 0; q < nb; q++) rank += (int)(bound[q] < b);
		run_start[rank] = b;
	}
	__syncthreads();
	const int run = blockIdx.x;
	if (run >= runs) return;
	const int s0 = run_start[run], n = run_start[run + 1] - s0;
	int item0 = 0, items = 0;
	for (int q = 0; q < runs; q++) { if (q == run) item0 = items; items += (run_start[q + 1] - run_start[q] + 1) >> 1; }
	if (run == 0 && tid == 0) { bo.ctl[0] = items; bo.ctl[1] = 1; bo.ctl[2] = 0; bo.ctl[3] = 0; bo.ctl[kBoundsCopies] = 0; if (bo.host_note) *bo.host_note = (long long)G << 1; }
	if (run == 0 && tid < 64) bounds_cuts_store(bo, balanced, items, tid);
	// the extent of the run's centres (a thread without a k-th group holds the run's last one again: it changes neither the extent nor, below, a counter)
	float held[kOrderHeld][3];
	float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
	for (int h = 0; h < kOrderHeld; h++) group_centre(cubes, s0 + min(tid + h * 1024, n - 1), B, held[h]);
#pragma unroll
	for (int h = 0; h < kOrderHeld; h++) {
#pragma unroll
		for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], held[h][k]); hi[k] = fmaxf(hi[k], held[h][k]); }
	}
	for (int j = tid + kOrderHeld * 1024; j < n; j += 1024) {
		float c[3];
		group_centre(cubes, s0 + j, B, c);
#pragma unroll
		for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], c[k]); hi[k] = fmaxf(hi[k], c[k]); }
	}
#pragma unroll
	for (int k = 0; k < 3; k++) {
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64)); }
		if (lane == 0) { ext[wave][k] = lo[k]; ext[wave][3 + k] = hi[k]; }
	}
	__syncthreads();
	float span = 0.f;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		for (int w = 0; w < 16; w++) { lo[k] = fminf(lo[k], ext[w][k]); hi[k] = fmaxf(hi[k], ext[w][3 + k]); }
		span = fmaxf(span, hi[k] - lo[k]);
	}
	const float cell = fmaxf(fmaxf(bo.cell_vox, 1.f), span * dt.scale_f * (1.f / 31.5f));   // voxels; 32 cells cover the span
	const float to_cell = dt.scale_f / cell;
	unsigned key[kOrderHeld];
#pragma unroll
	for (int h = 0; h < kOrderHeld; h++) {
		key[h] = order_key(held[h], lo, to_cell);
		if (tid + h * 1024 < n) atomicAdd(&lds[key[h] + key[h] / per], 1u);
	}
	for (int j = tid + kOrderHeld * 1024; j < n; j += 1024) {
		float c[3];
		group_centre(cubes, s0 + j, B, c);
		const unsigned kj = order_key(c, lo, to_cell);
		atomicAdd(&lds[kj + kj / per], 1u);
	}
	__syncthreads();
	// exclusive scan of the 32 768 counters
	const int b0 = tid * (per + 1);
	unsigned local = 0;
#pragma unroll
	for (int k = 0; k < per; k++) local += lds[b0 + k];
	unsigned incl = local;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
	if (lane == 63) wtot[wave] = incl;
	__syncthreads();
	unsigned before = 0;
	for (int w = 0; w < wave; w++) before += wtot[w];
	unsigned runsum = before + incl - local;
#pragma unroll
	for (int k = 0; k < per; k++) { const unsigned c = lds[b0 + k]; lds[b0 + k] = runsum; runsum += c; }
	__syncthreads();
	// slot `pos` of the run's order: order[] and the pos-th member of the run's pair list; a leftover's partner is -1
	auto place = [&](unsigned kj, int j) {
		const int pos = (int)atomicAdd(&lds[kj + kj / per], 1u), it = item0 + (pos >> 1);
		bo.order[s0 + pos] = (unsigned)(s0 + j);
		bo.pairs[2 * it + (pos & 1)] = s0 + j;
		if (pos == n - 1 && !(pos & 1)) bo.pairs[2 * it + 1] = -1;
	};
#pragma unroll
	for (int h = 0; h < kOrderHeld; h++)
		if (tid + h * 1024 < n) place(key[h], tid + h * 1024);
	for (int j = tid + kOrderHeld * 1024; j < n; j += 1024) {
		float c[3];
		group_centre(cubes, s0 + j, B, c);
		place(order_key(c, lo, to_cell), j);
	}
	// Copies (BoundsOrder::alias): the counters are dead now and serve as an open-addressing table over the run's full groups, two 64-bit
	// slots per group up to the 16 384 that fit.  A group hashes its children 0 and 7, claims the first empty slot of its probe sequence with a
	// compare-and-swap of (hash, index), and on the way compares all eight of its records with those of every occupant of its hash, word for
	// word: equal, and the occupant is its owner.  An occupant has claimed a slot, hence is its own owner; a partial last group neither claims nor compares; a group
	// that saw kBoundsAliasProbes slots taken by others stays its own owner unlisted.  Which listing of a family owns it follows the atomics:
	// no bound depends on it, a copy takes the sums of an evaluation of the very records it holds.
	if (!bo.alias) return;
	__syncthreads();
	// an entry is (hash << 32 | index in the run): an occupant of another hash is passed without a look at its records
	unsigned long long* table = reinterpret_cast<unsigned long long*>(lds);
	int slots = 64;
	while (slots < 2 * n && slots < kSortBins / 2) slots <<= 1;
	for (int i = tid; i < slots / 2; i += 1024) reinterpret_cast<uint4*>(lds)[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
	__syncthreads();
	for (int j = tid; j < n; j += 1024) {
		const int g = s0 + j;
		int owner = g;
		if (g * kGroup + kGroup <= B) {
			const unsigned h = alias_hash(cubes[(size_t)g * kGroup], cubes[(size_t)g * kGroup + kGroup - 1]);
			const unsigned long long mine = ((unsigned long long)h << 32) | (unsigned)j;     // never all ones: j < 2^31
			unsigned slot = h & (unsigned)(slots - 1);
			for (int probe = 0; probe < kBoundsAliasProbes; probe++) {
				const unsigned long long old = atomicCAS(&table[slot], ~0ull, mine);
				if (old == ~0ull) break;
				if ((unsigned)(old >> 32) == h && same_records(cubes, g, s0 + (int)(unsigned)old)) { owner = s0 + (int)(unsigned)old; break; }
				slot = (slot + 1) & (unsigned)(slots - 1);
			}
		}
		bo.alias[g] = owner;
	}
}

// the plain launch walking order[] when the pre-pass built one (bounds_order = 1): bounds_kernel<1, true> with the slot -> group table.
// gate is 1 in the one launch there is; 0 (leave at once when there is an order) served a second launch after bounds_pair_kernel, which
// evaluates the batches the pre-pass leaves alone itself now.  The argument stays: without it the compiler spills 38 SGPRs here, not 24.
template <bool TRUNC>
__global__ __launch_bounds__(kBoundsThreads) void bounds_ordered_kernel(
    const float4* __restrict__ src, int N, DtDesc dt, const Rot9* __restrict__ rots,
    const CubeRec* __restrict__ cubes, const ParentRec* __restrict__ parents, int B, int groups, int chunks, int chunk_pts,
    float* __restrict__ scratch, float* __restrict__ ub_out, float* __restrict__ lb_out, const unsigned* __restrict__ order, const int* __restrict__ ctl, int gate)
{
	__shared__ float red[kBoundsThreads / 64][2 * kGroup];
	int work = blockIdx.x;
	if (ctl[1]) {
		if (!gate) return;
		int group, chunk;
		bounds_item_of(work, gridDim.x, groups, chunks, group, chunk);
		work = bounds_work_of((int)order[group], chunk, groups, chunks);
	}
	bounds_work<1, true, TRUNC>(work, gridDim.x, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub_out, lb_out, red);
}

// one member of a pair item: is the group a sibling set, and then its two translations per axis, its delta and coefficient
__device__ __forceinline__ bool pair_member(const CubeRec* __restrict__ cubes, const ParentRec* __restrict__ parents, int group, int B, PairMember& m, int& rot)
{
	CubeRec cr[kGroup];
	load_group(cubes, parents, group, B, cr);
	bool sib = group * kGroup + kGroup <= B;
#pragma unroll
	for (int c = 0; c < kGroup; c++)
		sib = sib && cr[c].rot == cr[0].rot && cr[c].tx == cr[c & 1].tx && cr[c].ty == cr[c & 2].ty && cr[c].tz == cr[c & 4].tz &&
		      cr[c].delta == cr[0].delta && cr[c].coeff == cr[0].coeff;
	m.ts = SiblingSet{cr[0].tx, cr[1].tx, cr[0].ty, cr[2].ty, cr[0].tz, cr[4].tz};
	m.delta = cr[0].delta; m.coeff = cr[0].coeff; rot = cr[0].rot;
	return sib;
}
// do two members look up the same voxels under every point?  raw bits: -0 against +0 is no match and keeps the pair form
__device__ __forceinline__ bool same_box(const PairMember& a, const PairMember& b)
{
	const unsigned d = (__float_as_uint(a.ts.tx0) ^ __float_as_uint(b.ts.tx0)) | (__float_as_uint(a.ts.tx1) ^ __float_as_uint(b.ts.tx1)) |
	                   (__float_as_uint(a.ts.ty0) ^ __float_as_uint(b.ts.ty0)) | (__float_as_uint(a.ts.ty1) ^ __float_as_uint(b.ts.ty1)) |
	                   (__float_as_uint(a.ts.tz0) ^ __float_as_uint(b.ts.tz0)) | (__float_as_uint(a.ts.tz1) ^ __float_as_uint(b.ts.tz1)) |
	                   (__float_as_uint(a.delta) ^ __float_as_uint(b.delta));
	return d == 0u;
}
// the pair launch (bounds_order = 2): grid = max_items * chunks, an item = the two groups pairs[] names over one chunk, mapped to the XCDs as bounds_work maps (group, chunk).  Two sibling sets of one rotation are evaluated together
// (lean_points_pair); anything else -- a generic group, a partial last group, a foreign rotation, a single -- group by group on the plain path.
// COINCIDENT members -- the six translations and delta equal as raw bits: the root expansion of every inner search, the node both searches of a
// rotation child list; the pre-pass puts them in one cell, hence next to each other -- have the same addresses: such an item runs
// lean_points<1, 2, ..> once (the loop of the queue twins), or, with equal coefficients too, lean_points<1, 1, ..> once for both groups' rows.
// Thread 0 of the item's chunk-0 workgroup counts the form in ctl[2] / ctl[3] (goicp_debug_bounds_twins).
// COPIES -- a family listed more than twice is more than one item: over several chunks a member the pre-pass found to repeat another group
// of its run record for record (alias[g] != g) is not evaluated at all, the other member goes alone on the plain path, and bounds_finalize
// takes the copy's bounds from its owner's rows; the forms are tallied first, from the records, and ctl[kBoundsCopies] counts the copies.
// A batch the pre-pass left alone (ctl[1] = 0) is evaluated here too, two groups per item in arrival order on the plain path: the grid of
// bounds_order_items(groups, max_runs) >= (groups + 1) / 2 items covers it, and no second launch is needed.
// The 8-chunk shape (chunks == 8) takes its units from the cuts the pre-pass left behind ctl[0..3] (bounds_cuts): block label x = work & 7
// evaluates the units cut[x] .. cut[x + 1] - 1 of the chunk-major list u = chunk * items + item, so a label whose chunk gathers more lines per
// wavefront hands the tail of its chunk to its neighbour.  The map is a bijection of the blocks below cut[x + 1] - cut[x] per label onto the
// units whatever XCD a label lands on; the grid is 8 * bounds_pair_slots(max_items) and the surplus leaves at once.  Equal cuts
// (cut[x] = x * items: bounds_balance = 0, a batch the pre-pass left alone included) are the static map chunk = x.
#ifdef GOICP_BOUNDS_XCD_STAMPS
// diagnostic build only (make stamps): the kernel below becomes the body of a kernel that stamps its entry and exit per XCC
#define GOICP_BOUNDS_PAIR_HEAD __device__ __forceinline__ void bounds_pair_body
#else
#define GOICP_BOUNDS_PAIR_HEAD __global__ __launch_bounds__(kBoundsThreads) void bounds_pair_kernel
#endif
template <bool TRUNC>
GOICP_BOUNDS_PAIR_HEAD(
    const float4* __restrict__ src, int N, DtDesc dt, const Rot9* __restrict__ rots,
    const CubeRec* __restrict__ cubes, const ParentRec* __restrict__ parents, int B, int groups, int max_items, int chunks, int chunk_pts,
    float* __restrict__ scratch, float* __restrict__ ub_out, float* __restrict__ lb_out, const int* __restrict__ pairs, int* __restrict__ ctl,
    const int* __restrict__ alias)
{
	__shared__ float red[kBoundsThreads / 64][2 * kGroup];
	const int work = blockIdx.x, total = gridDim.x;
	int chunk, item;
	if (chunks == 8) {
		const int xcd = work & 7, u = ctl[kBoundsCut + xcd] + (work >> 3);
		if (u >= ctl[kBoundsCut + xcd + 1]) return;
		const int items = ctl[kBoundsCut + 8] >> 3;          // cut[8] = 8 * items
		chunk = u / items;
		item = u - chunk * items;
	} else if ((chunks & 7) == 0) {
		const int cpx = chunks >> 3, xcd = work & 7, slot = work >> 3;
		item = slot / cpx;
		chunk = xcd * cpx + (slot - item * cpx);
	} else {
		const int swz = xcd_remap(work, total);
		chunk = swz / max_items; item = swz - chunk * max_items;
	}
	const bool listed = ctl[1] != 0;
	int ga, gb;
	if (listed) {
		if (item >= ctl[0]) return;
		ga = pairs[2 * item]; gb = pairs[2 * item + 1];
	} else {                                             // the pre-pass left the batch alone: groups 2 item and 2 item + 1 as they came, each on the plain path
		ga = 2 * item;
		if (ga >= groups) return;
		gb = ga + 1 < groups ? ga + 1 : -1;
	}
	// members the pre-pass found to be copies of another group of their run (BoundsOrder::alias; several chunks only, where bounds_finalize
	// sums a copy's bounds from its owner's rows): bit 0 the first, bit 1 the second.  Counted like the forms, by the item's chunk-0 workgroup
	int copy = 0;
	if (listed && alias && chunks > 1) {
		copy = (alias[ga] != ga ? 1 : 0) | (gb >= 0 && alias[gb] != gb ? 2 : 0);
		if (copy && chunk == 0 && threadIdx.x == 0) atomicAdd(ctl + kBoundsCopies, (copy & 1) + (copy >> 1));
	}
	if (listed && gb >= 0) {
		PairMember A, Bm;
		int ra, rb;
		const bool sa = pair_member(cubes, parents, ga, B, A, ra), sb = pair_member(cubes, parents, gb, B, Bm, rb);
		const bool both = sa && sb && ra == rb;
		// the forms are tallied from the records, whatever is evaluated below
		if (both && chunk == 0 && threadIdx.x == 0 && same_box(A, Bm))
			atomicAdd(ctl + (__float_as_uint(A.coeff) == __float_as_uint(Bm.coeff) || (A.coeff == 0.f && Bm.coeff == 0.f) ? 3 : 2), 1);
		if (both && !copy) {
			const Rot9 R0 = rots[ra];
			const int p0 = chunk * chunk_pts;
			const int p1 = p0 + chunk_pts < N ? p0 + chunk_pts : N;
			if (same_box(A, Bm)) {
				// coincident members: one index set, one exactness test and one set of gathers per point serve both (lean_points, which has
				// its own checked branch: nothing is given up here); a pass of the NP = 2 loop is a separate evaluation operation for operation
				const bool same = __float_as_uint(A.coeff) == __float_as_uint(Bm.coeff) || (A.coeff == 0.f && Bm.coeff == 0.f);
				float ub[kGroup], lb[kGroup];
				if (same) {                                       // the same expansion twice: evaluated once, stored to both groups' rows
					f2 ub2[1][4], lb2[1][4];
#pragma unroll
					for (int k = 0; k < 4; k++) { ub2[0][k] = f2{0.f, 0.f}; lb2[0][k] = f2{0.f, 0.f}; }
					const float co[1] = {A.coeff};
					if (A.coeff == 0.f) lean_points<1, 1, true, TRUNC>(src, p0, p1, dt, R0, A.ts, A.delta, co, ub2, lb2);
					else lean_points<1, 1, false, TRUNC>(src, p0, p1, dt, R0, A.ts, A.delta, co, ub2, lb2);
#pragma unroll
					for (int k = 0; k < 4; k++) { ub[2 * k] = ub2[0][k].x; ub[2 * k + 1] = ub2[0][k].y; lb[2 * k] = lb2[0][k].x; lb[2 * k + 1] = lb2[0][k].y; }
					bounds_item_store(ub, lb, ga, chunk, chunks, B, scratch, ub_out, lb_out, red, gb);
					return;
				}
				if (A.coeff == 0.f) {                             // the member without a rotation radius goes last (LAST_ZERO)
					const float c = A.coeff; A.coeff = Bm.coeff; Bm.coeff = c;
					const int g = ga; ga = gb; gb = g;
				}
				f2 ub2[2][4], lb2[2][4];
#pragma unroll
				for (int q = 0; q < 2; q++)
#pragma unroll
					for (int k = 0; k < 4; k++) { ub2[q][k] = f2{0.f, 0.f}; lb2[q][k] = f2{0.f, 0.f}; }
				const float co[2] = {A.coeff, Bm.coeff};
				if (Bm.coeff == 0.f) lean_points<1, 2, true, TRUNC>(src, p0, p1, dt, R0, A.ts, A.delta, co, ub2, lb2);
				else lean_points<1, 2, false, TRUNC>(src, p0, p1, dt, R0, A.ts, A.delta, co, ub2, lb2);
#pragma unroll
				for (int k = 0; k < 4; k++) { ub[2 * k] = ub2[1][k].x; ub[2 * k + 1] = ub2[1][k].y; lb[2 * k] = lb2[1][k].x; lb[2 * k + 1] = lb2[1][k].y; }
				bounds_item_store(ub, lb, gb, chunk, chunks, B, scratch, ub_out, lb_out, red);
				__syncthreads();                                  // `red` is reused
#pragma unroll
				for (int k = 0; k < 4; k++) { ub[2 * k] = ub2[0][k].x; ub[2 * k + 1] = ub2[0][k].y; lb[2 * k] = lb2[0][k].x; lb[2 * k + 1] = lb2[0][k].y; }
				bounds_item_store(ub, lb, ga, chunk, chunks, B, scratch, ub_out, lb_out, red);
				return;
			}
			if (A.coeff != 0.f && Bm.coeff == 0.f) {       // at most one member without a rotation radius: make it the first (LZ_A)
				const PairMember t = A; A = Bm; Bm = t;
				const int g = ga; ga = gb; gb = g;
			}
			f2 ubA[4], lbA[4], ubB[4], lbB[4];
#pragma unroll
			for (int k = 0; k < 4; k++) { ubA[k] = f2{0.f, 0.f}; lbA[k] = f2{0.f, 0.f}; ubB[k] = f2{0.f, 0.f}; lbB[k] = f2{0.f, 0.f}; }
			bool okA = true, okB = true;
			if (A.coeff == 0.f && Bm.coeff == 0.f) lean_points_pair<true, true, TRUNC>(src, p0, p1, dt, R0, A, Bm, ubA, lbA, ubB, lbB, okA, okB);
			else if (A.coeff == 0.f) lean_points_pair<true, false, TRUNC>(src, p0, p1, dt, R0, A, Bm, ubA, lbA, ubB, lbB, okA, okB);
			else lean_points_pair<false, false, TRUNC>(src, p0, p1, dt, R0, A, Bm, ubA, lbA, ubB, lbB, okA, okB);
			// some wavefront gave a member up: its sums are void in all four (the barrier hands back a predicate, so one per member)
			const int bad = (__syncthreads_or(okA ? 0 : 1) ? 1 : 0) | (__syncthreads_or(okB ? 0 : 1) ? 2 : 0);
			float ub[kGroup], lb[kGroup];
			if (!(bad & 1)) {
#pragma unroll
				for (int k = 0; k < 4; k++) { ub[2 * k] = ubA[k].x; ub[2 * k + 1] = ubA[k].y; lb[2 * k] = lbA[k].x; lb[2 * k + 1] = lbA[k].y; }
				bounds_item_store(ub, lb, ga, chunk, chunks, B, scratch, ub_out, lb_out, red);
				__syncthreads();                              // `red` is reused
			}
			if (!(bad & 2)) {
#pragma unroll
				for (int k = 0; k < 4; k++) { ub[2 * k] = ubB[k].x; ub[2 * k + 1] = ubB[k].y; lb[2 * k] = lbB[k].x; lb[2 * k + 1] = lbB[k].y; }
				bounds_item_store(ub, lb, gb, chunk, chunks, B, scratch, ub_out, lb_out, red);
				__syncthreads();
			}
			if (bad == 0) return;
			if (!(bad & 1)) ga = gb;                          // what is left for the plain path: the member given up, or both
			if (bad != 3) gb = -1;
		}
	}
	if (copy & 2) gb = -1;                                // a copy is not evaluated: the other member goes alone, or the workgroup leaves
	if (copy & 1) { ga = gb; gb = -1; }
#pragma unroll 1
	for (int m = 0; m < 2; m++) {
		const int g = m ? gb : ga;
		if (g < 0) break;
		if (m) __syncthreads();
		bounds_work<1, true, TRUNC>(bounds_work_of(g, chunk, groups, chunks), groups * chunks, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub_out, lb_out, red);
	}
}
#undef GOICP_BOUNDS_PAIR_HEAD
#ifdef GOICP_BOUNDS_XCD_STAMPS
// Per XCC (HW_REG_XCC_ID, the physical XCD) and per block label (work & 7): the first entry and the last exit of a workgroup on the 100 MHz
// clock, the workgroups, the sum of their times, and for the XCC rows a mask of the labels seen there.  Thread 0 stamps; the barrier makes its
// exit stamp the workgroup's (every return of the body is taken by the whole workgroup).
constexpr int kXcdStampStride = 16;                  // a row per 128-B line: the rows do not contend with each other
__device__ unsigned long long g_xcd_stamps[kXcdStampRows * kXcdStampStride];
template <bool TRUNC>
__global__ __launch_bounds__(kBoundsThreads) void bounds_pair_kernel(
    const float4* __restrict__ src, int N, DtDesc dt, const Rot9* __restrict__ rots,
    const CubeRec* __restrict__ cubes, const ParentRec* __restrict__ parents, int B, int groups, int max_items, int chunks, int chunk_pts,
    float* __restrict__ scratch, float* __restrict__ ub_out, float* __restrict__ lb_out, const int* __restrict__ pairs, int* __restrict__ ctl,
    const int* __restrict__ alias)
{
	const unsigned long long t0 = wall_clock64();
	bounds_pair_body<TRUNC>(src, N, dt, rots, cubes, parents, B, groups, max_items, chunks, chunk_pts, scratch, ub_out, lb_out, pairs, ctl, alias);
	__syncthreads();
	if (threadIdx.x == 0) {
		const unsigned long long t1 = wall_clock64();
		const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u;      // hwreg(HW_REG_XCC_ID, 0, 4)
		const unsigned rows[2] = {xcc, 8u + (blockIdx.x & 7u)};
		for (int k = 0; k < 2; k++) {
			unsigned long long* s = g_xcd_stamps + rows[k] * kXcdStampStride;
			if (t1 - t0 < 100ull) { atomicAdd(s + 5, 1ull); continue; }           // under 1 us: a surplus workgroup that left at once
			atomicMin(s + 0, t0); atomicMax(s + 1, t1); atomicAdd(s + 2, 1ull); atomicAdd(s + 3, t1 - t0);
		}
		atomicOr(g_xcd_stamps + xcc * kXcdStampStride + 4, 1ull << (blockIdx.x & 7u));
	}
}
#endif

// The same evaluation for a batch whose size only the DEVICE knows (the device-resident BnB queues, bnbqueue.hip):
// *d_groups expansions of 8 children each; a fixed grid walks the (group, chunk) work items, the split of the cloud
// into chunks follows from the count exactly as on the host (bounds_shape).  ub_out / lb_out: [8 * groups] each.
__host__ __device__ inline void bounds_shape(int B, int N, int* groups, int* chunks, int* chunk_pts);
// Work distribution: a launch of exactly-sized grids lets the hardware hand the next block to whichever CU frees up;
// a fixed grid that strides statically over the items loses that (measured on the full bunny: 22.2 ms of bound
// evaluation against 15 ms -- item counts like 3.2 per block leave a quarter of the chip idle in the last pass).
// So the fixed grid draws its items dynamically: eight counters, one per XCD slot (blocks b and b+8 share an XCD), each
// handing out the items whose index is congruent to that slot -- the XCD-aware tiling of bounds_work is kept, and the
// fetch of the next item overlaps the evaluation of the current one.
template <int LAYOUT, bool LEAN = false, bool TRUNC = false>
__global__ __launch_bounds__(kBoundsThreads) void bounds_queue_kernel(
    const float4* __restrict__ src, int N, DtDesc dt, const Rot9* __restrict__ rots, const ParentRec* __restrict__ parents,
    const int* __restrict__ d_groups, int* __restrict__ work8, int* __restrict__ d_chunks, float* __restrict__ scratch, float* __restrict__ ub_out,
    float* __restrict__ lb_out, const QSearch* __restrict__ searches, const int* __restrict__ parent_search, QSort qs)
{
	__shared__ float red[kBoundsThreads / 64][2 * kGroup];
	__shared__ int next_item[2];
	__shared__ int twin_sh;
	const TwinCtx twin{LEAN ? searches : nullptr, parent_search, &twin_sh};
	const int ngroups = *d_groups;
	if (ngroups <= 0) return;
	int groups, chunks, chunk_pts;
	const bool sorted = qsort_on(qs, ngroups);
	if (sorted) { groups = ngroups; chunks = qs.chunks; chunk_pts = qs.chunk_pts; }
	else bounds_shape(ngroups * kGroup, N, &groups, &chunks, &chunk_pts);
	if (blockIdx.x == 0 && threadIdx.x == 0) *d_chunks = chunks;          // > 1: the next round's digest adds the chunk partials up
	if (sorted)                                                           // the order is built: leave the histogram zeroed for the next sorted round
		for (int i = blockIdx.x * kBoundsThreads + threadIdx.x; i < kSortBins; i += gridDim.x * kBoundsThreads) qs.hist[i] = 0u;
	const int total = groups * chunks;
	const bool per_xcd = sorted || (total & 7) == 0;
	const int slot = per_xcd ? (int)(blockIdx.x & 7) : 0, stride = per_xcd ? 8 : 1;
	int* ctr = work8 + slot;
	if (threadIdx.x == 0) next_item[0] = atomicAdd(ctr, 1);
	__syncthreads();
	int item = next_item[0], buf = 0;
	while (item * stride + slot < total) {
		if (threadIdx.x == 0) next_item[buf ^ 1] = atomicAdd(ctr, 1);   // in flight while this item is evaluated
		bounds_work<LAYOUT, LEAN, TRUNC>(item * stride + slot, total, src, N, dt, rots, nullptr, parents, ngroups * kGroup, groups, chunks, chunk_pts, scratch, ub_out,
		                    lb_out, red, sorted ? qs.order : nullptr, twin);
		__syncthreads();                                                 // `red` is reused by the next item; next_item is published
		buf ^= 1;
		item = next_item[buf];
	}
}

// alias, ctl: null, or the pair launch's (BoundsOrder::alias, ::ctl): with an order in force (ctl[1]) the rows of group g are those of alias[g],
// the group evaluated in its place -- the same fixed chunk order over the sums of the same eight records
__global__ void bounds_finalize(const float* __restrict__ scratch, int B, int groups, int chunks,
                                float* __restrict__ ub_out, float* __restrict__ lb_out, const int* __restrict__ alias, const int* __restrict__ ctl)
{
	int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= groups * 2 * kGroup) return;
	int group = t / (2 * kGroup), k = t - group * 2 * kGroup;
	int c = group * kGroup + (k & (kGroup - 1));
	if (c >= B) return;
	const int rows = alias && ctl[1] ? alias[group] : group;
	const float* s = scratch + (size_t)rows * chunks * (2 * kGroup) + k;
	float acc = 0.f;
	for (int j = 0; j < chunks; j++) acc += s[(size_t)j * 2 * kGroup];
	(k < kGroup ? ub_out : lb_out)[c] = acc;
}

// ------------------------------------------------------------------------------------------------
// Trimmed cube bounds (trimFraction > 0; jly_goicp.cpp:293-315): only the `inliers` smallest clamped
// residuals of a cube enter the two sums.  One workgroup owns 8 cubes and ALL points; the k-th
// smallest residual of each cube is found exactly by a 3-digit radix select on the float bit
// pattern (11+11+9 bits, integer LDS histograms -> deterministic), recomputing the residuals in
// every pass instead of storing B x N floats; a fourth pass sums the residuals below the threshold
// T, and the `rem` copies of T itself are added once.
// ------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads per expansion: it sweeps the whole cloud four times, and with a single
// workgroup per CU only its own wavefronts can hide the gather latency.
constexpr int kTrimThreads = 1024;
template <int LAYOUT>
__global__ __launch_bounds__(kTrimThreads) void bounds_trim_kernel(
    const float4* __restrict__ src, int N, DtDesc dt, const Rot9* __restrict__ rots,
    const CubeRec* __restrict__ cubes, const ParentRec* __restrict__ parents, int B, int inliers,
    float* __restrict__ ub_out, float* __restrict__ lb_out, const int* __restrict__ d_groups, int* __restrict__ d_chunks = nullptr)
{
	if (d_groups) {                           // batch size known to the device only (device-resident BnB queues)
		if (d_chunks && blockIdx.x == 0 && threadIdx.x == 0) *d_chunks = 1;     // this form writes the final bounds itself
		if ((int)blockIdx.x >= *d_groups) return;
		B = *d_groups * kGroup;
	}
	__shared__ unsigned hist[kGroup][2048];
	__shared__ unsigned sel_prefix[kGroup], sel_rem[kGroup];
	__shared__ float red[kTrimThreads / 64][2 * kGroup];
	const int c0 = blockIdx.x * kGroup;
	CubeRec cr[kGroup];
	load_group(cubes, parents, blockIdx.x, B, cr);
	if (threadIdx.x < kGroup) { sel_prefix[threadIdx.x] = 0u; sel_rem[threadIdx.x] = (unsigned)inliers; }

	// the 8 clamped residuals of one point: the sibling form (one rotation, 6 voxel indices) for an expansion,
	// the per-cube form for anything else; same values either way
	const bool sib = is_sibling_set(cr) && c0 + kGroup <= B;
	const Rot9 R0 = rots[cr[0].rot];
	const SiblingSet ts{cr[0].tx, cr[1].tx, cr[0].ty, cr[2].ty, cr[0].tz, cr[4].tz};
	auto residuals = [&](const float4& p, float m[kGroup]) {
		if (sib) { sibling_residuals<LAYOUT>(dt, R0, ts, p, cr[0].coeff * p.w, m); return; }
#pragma unroll
		for (int c = 0; c < kGroup; c++) {
			const Rot9 R = rots[cr[c].rot];
			const float rx = R.r[0] * p.x + R.r[1] * p.y + R.r[2] * p.z;
			const float ry = R.r[3] * p.x + R.r[4] * p.y + R.r[5] * p.z;
			const float rz = R.r[6] * p.x + R.r[7] * p.y + R.r[8] * p.z;
			float v = dt_distance<LAYOUT>(dt, rx + cr[c].tx, ry + cr[c].ty, rz + cr[c].tz);
			v = v - cr[c].coeff * p.w;
			m[c] = v < 0.f ? 0.f : v;
		}
	};

#pragma unroll 1
	for (int pass = 0; pass < 3; pass++) {
		const int shift = pass == 0 ? 20 : (pass == 1 ? 9 : 0), width = pass == 2 ? 9 : 11, bins = 1 << width;
		for (int i = threadIdx.x; i < kGroup * 2048; i += kTrimThreads) (&hist[0][0])[i] = 0u;
		__syncthreads();
		for (int i = threadIdx.x; i < N; i += kTrimThreads) {
			const float4 p = src[i];
			float m[kGroup];
			residuals(p, m);
#pragma unroll
			for (int c = 0; c < kGroup; c++) {
				const unsigned key = __float_as_uint(m[c]);
				if (pass == 0 || (key >> (shift + width)) == sel_prefix[c])
					atomicAdd(&hist[c][(key >> shift) & (unsigned)(bins - 1)], 1u);
			}
		}
		__syncthreads();
		// 32 threads per cube (the first four wavefronts): locate the bin holding the rem-th smallest of the
		// surviving candidates
		if (threadIdx.x < 32 * kGroup) {
			const int c = threadIdx.x >> 5, j = threadIdx.x & 31, per = bins >> 5;
			unsigned local = 0;
			for (int b = j * per; b < (j + 1) * per; b++) local += hist[c][b];
			unsigned incl = local;
#pragma unroll
			for (int off = 1; off < 32; off <<= 1) {
				const unsigned o = __shfl_up(incl, off, 32);
				if (j >= off) incl += o;
			}
			const unsigned excl = incl - local, rem = sel_rem[c];
			if (excl < rem && rem <= incl) {
				unsigned cum = excl;
				for (int b = j * per; b < (j + 1) * per; b++) {
					const unsigned h = hist[c][b];
					if (cum < rem && rem <= cum + h) {
						sel_prefix[c] = (sel_prefix[c] << width) | (unsigned)b;
						sel_rem[c] = rem - cum;
						break;
					}
					cum += h;
				}
			}
		}
		__syncthreads();
	}

	float ub[kGroup], lb[kGroup];
#pragma unroll
	for (int c = 0; c < kGroup; c++) { ub[c] = 0.f; lb[c] = 0.f; }
	for (int i = threadIdx.x; i < N; i += kTrimThreads) {
		const float4 p = src[i];
		float m[kGroup];
		residuals(p, m);
#pragma unroll
		for (int c = 0; c < kGroup; c++) {
			if (__float_as_uint(m[c]) < sel_prefix[c]) {     // strictly below the k-th smallest
				ub[c] += m[c] * m[c];
				const float dis = fmaxf(m[c] - cr[c].delta, 0.f);
				lb[c] += dis * dis;
			}
		}
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int c = 0; c < kGroup; c++) {
		const float u = wave_sum(ub[c]), l = wave_sum(lb[c]);
		if (lane == 0) { red[wave][c] = u; red[wave][kGroup + c] = l; }
	}
	__syncthreads();
	if (threadIdx.x < 2 * kGroup) {
		float s = red[0][threadIdx.x];
#pragma unroll
		for (int w = 1; w < kTrimThreads / 64; w++) s += red[w][threadIdx.x];
		const int c = threadIdx.x & (kGroup - 1);
		// the residuals equal to the threshold: sel_rem copies of T
		const float T = __uint_as_float(sel_prefix[c]);
		const float n_eq = (float)sel_rem[c];
		if (threadIdx.x < kGroup) s += n_eq * (T * T);
		else {
			const float delta_c = parents ? cr[0].delta : cubes[c0 + c < B ? c0 + c : B - 1].delta;   // read, not cr[c]: no dynamic register indexing
			const float dis = fmaxf(T - delta_c, 0.f);
			s += n_eq * (dis * dis);
		}
		if (c0 + c < B) (threadIdx.x < kGroup ? ub_out : lb_out)[c0 + c] = s;
	}
}

hipError_t launch_bounds_trim(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const CubeRec* cubes, const ParentRec* parents, int B,
                              int inliers, float* ub, float* lb, hipStream_t stream)
{
	if (B <= 0 || N <= 0) return hipSuccess;
	const dim3 grid((B + kGroup - 1) / kGroup), block(kTrimThreads);
	if (dt.layout == 2) return hipErrorInvalidValue;          // the trimmed form is evaluated on the fp32 grid
	if (dt.layout == 0) hipLaunchKernelGGL(bounds_trim_kernel<0>, grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, inliers, ub, lb, (const int*)nullptr, (int*)nullptr);
	else hipLaunchKernelGGL(bounds_trim_kernel<1>, grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, inliers, ub, lb, (const int*)nullptr, (int*)nullptr);
	return hipGetLastError();
}

__host__ __device__ inline void bounds_shape(int B, int N, int* groups, int* chunks, int* chunk_pts)
{
	int g = (B + kGroup - 1) / kGroup;
	// aim for >= 4 blocks of 256 threads per CU (256 CUs) even for small batches, and
	// for a multiple of 8 point chunks (one set per XCD) whenever the cloud is large enough
	const int target_blocks = 1024;   // measured on the BnB's small batches: 512..2048 within 5 %, larger is slower
	const int max_chunks = (N + kBoundsThreads - 1) / kBoundsThreads;
	int c = (target_blocks + g - 1) / g;
	// eight chunk sets only when each of them still gets >= 4 iterations of 256 points: a workgroup's fixed cost (cube records,
	// reduction, partial row) is spread over too few points otherwise (bunny/10, N = 3 038: 8 chunks of 380 points)
	const bool sets = max_chunks >= 32;
	if (sets) c = (c + 7) / 8 * 8;
	if (c > max_chunks) c = sets ? max_chunks / 8 * 8 : max_chunks;
	if (c < 1) c = 1;
	int cp = (N + c - 1) / c;
	cp = (cp + kBoundsThreads - 1) / kBoundsThreads * kBoundsThreads;
	int c2 = (N + cp - 1) / cp;                 // rounding the chunk size up may empty the last chunks
	if (sets && (c & 7) == 0 && c2 != c) { /* keep c: trailing chunks are simply empty */ } else c = c2;
	*groups = g; *chunks = c; *chunk_pts = cp;
}

size_t bounds_scratch_floats(int B, int N, int* groups_out, int* chunks_out)
{
	int g, c, cp;
	bounds_shape(B, N, &g, &c, &cp);
	if (groups_out) *groups_out = g;
	if (chunks_out) *chunks_out = c;
	return (size_t)g * c * 2 * kGroup;
}

size_t bounds_queue_scratch_floats(int max_groups, int sorted_chunks)
{
	// groups x chunks partial rows: chunks <= 8 + 1024/groups (bounds_shape), so groups*chunks <= 8*groups + 4096 (margin included);
	// footprint-ordered rounds cut the cloud into sorted_chunks chunks
	return (size_t)2 * kGroup * ((size_t)std::max(8, sorted_chunks) * (size_t)max_groups + 4096);
}

hipError_t launch_bounds_queue(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const ParentRec* parents, const int* d_groups,
                               int* d_work8, int* d_chunks, int max_groups, int inliers, float* scratch, float* ub, float* lb, hipStream_t stream,
                               const QSearch* searches, const int* parent_search, const QSort* qsort)
{
	if (!parent_search) searches = nullptr;
	QSort qs{};
	if (qsort && dt.layout == 1 && bounds_lean(dt) && inliers >= N) qs = *qsort;
	if (max_groups <= 0 || N <= 0) return hipSuccess;
	if (inliers < N) {
		// trimmed form: one workgroup per expansion, the surplus workgroups of the fixed grid leave at once
		const dim3 grid(max_groups), block(kTrimThreads);
		if (dt.layout == 2) return hipErrorInvalidValue;
		if (dt.layout == 0) hipLaunchKernelGGL(bounds_trim_kernel<0>, grid, block, 0, stream, src, N, dt, rots, (const CubeRec*)nullptr, parents, 0, inliers, ub, lb, d_groups, d_chunks);
		else hipLaunchKernelGGL(bounds_trim_kernel<1>, grid, block, 0, stream, src, N, dt, rots, (const CubeRec*)nullptr, parents, 0, inliers, ub, lb, d_groups, d_chunks);
		return hipGetLastError();
	}
	const dim3 grid(2048), block(kBoundsThreads);                        // 8 workgroups per CU, a multiple of 8 (XCD slots)
	if (dt.trunc > 0.f) {                                                // the truncated objective (DtDesc::trunc): the same four choices
		if (dt.layout == 0) hipLaunchKernelGGL((bounds_queue_kernel<0, false, true>), grid, block, 0, stream, src, N, dt, rots, parents, d_groups, d_work8, d_chunks, scratch, ub, lb, searches, parent_search, qs);
		else if (dt.layout == 1 && bounds_lean(dt)) hipLaunchKernelGGL((bounds_queue_kernel<1, true, true>), grid, block, 0, stream, src, N, dt, rots, parents, d_groups, d_work8, d_chunks, scratch, ub, lb, searches, parent_search, qs);
		else if (dt.layout == 1) hipLaunchKernelGGL((bounds_queue_kernel<1, false, true>), grid, block, 0, stream, src, N, dt, rots, parents, d_groups, d_work8, d_chunks, scratch, ub, lb, searches, parent_search, qs);
		else hipLaunchKernelGGL((bounds_queue_kernel<2, false, true>), grid, block, 0, stream, src, N, dt, rots, parents, d_groups, d_work8, d_chunks, scratch, ub, lb, searches, parent_search, qs);
		return hipGetLastError();
	}
	if (dt.layout == 0) hipLaunchKernelGGL(bounds_queue_kernel<0>, grid, block, 0, stream, src, N, dt, rots, parents, d_groups, d_work8, d_chunks, scratch, ub, lb, searches, parent_search, qs);
	else if (dt.layout == 1 && bounds_lean(dt)) hipLaunchKernelGGL((bounds_queue_kernel<1, true>), grid, block, 0, stream, src, N, dt, rots, parents, d_groups, d_work8, d_chunks, scratch, ub, lb, searches, parent_search, qs);
	else if (dt.layout == 1) hipLaunchKernelGGL(bounds_queue_kernel<1>, grid, block, 0, stream, src, N, dt, rots, parents, d_groups, d_work8, d_chunks, scratch, ub, lb, searches, parent_search, qs);
	else hipLaunchKernelGGL(bounds_queue_kernel<2>, grid, block, 0, stream, src, N, dt, rots, parents, d_groups, d_work8, d_chunks, scratch, ub, lb, searches, parent_search, qs);
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Footprint-ordered work items (round 3).  In the first rounds of a rotation batch every search expands whole levels of the
// translation tree: hundreds of rotations x all the cubes of a level, i.e. every rotation stamps the cloud all over the grid and
// sweeps the whole distance transform once.  Walked in search order, the items an XCD runs at any time gather from everywhere, its
// 4 MB L2 holds nothing for the next one, and the round runs at the Infinity Cache's bandwidth (a 128-byte line for every few
// 4-byte lookups; 75-110 CU cycles per gather against 37 when the lines are found in L2).  So for large rounds the (expansion, chunk)
// items are bucketed by WHERE their gathers land -- the Morton cell (16 voxels) of R * centroid(chunk) + centre(parent cube) -- with a
// counting sort (key + histogram, scan, scatter), XCD x walks the x-th eighth of the sorted list, and the cloud is cut into smaller
// chunks of 4 096 points (a ~90-voxel patch; the engine picks the size) so that an item's footprint stays compact.  The order changes no bound (an item's sums go to
// its own row); only the chunk count differs from the unsorted launch shape, i.e. the order in which a cube's per-chunk sums are added.
// Measured (tools/round_probe.py, bunny, 230 rotations, both passes): children of level 2 1.22 -> 1.04 ms, of level 3 8.87 -> 6.81 ms.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chunk_centroid_kernel(const float4* __restrict__ src, int N, int chunk_pts, float4* __restrict__ cen)
{
	__shared__ float red[4][3];
	const int p0 = blockIdx.x * chunk_pts, p1 = min(p0 + chunk_pts, N);
	float sx = 0.f, sy = 0.f, sz = 0.f;
	for (int i = p0 + (int)threadIdx.x; i < p1; i += 256) { const float4 p = src[i]; sx += p.x; sy += p.y; sz += p.z; }
	sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
	if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = sx; red[threadIdx.x >> 6][1] = sy; red[threadIdx.x >> 6][2] = sz; }
	__syncthreads();
	if (threadIdx.x == 0) {
		const float n = (float)max(p1 - p0, 1);
		cen[blockIdx.x] = make_float4((red[0][0] + red[1][0] + red[2][0] + red[3][0]) / n, (red[0][1] + red[1][1] + red[2][1] + red[3][1]) / n,
		                              (red[0][2] + red[1][2] + red[2][2] + red[3][2]) / n, 0.f);
	}
}
hipError_t launch_chunk_centroids(const float4* src, int N, int chunk_pts, float4* cen, hipStream_t stream)
{
	const int chunks = (N + chunk_pts - 1) / chunk_pts;
	hipLaunchKernelGGL(chunk_centroid_kernel, dim3(chunks), dim3(256), 0, stream, src, N, chunk_pts, cen);
	return hipGetLastError();
}
__global__ void task_key_kernel(const ParentRec* __restrict__ parents, const Rot9* __restrict__ rots, const int* __restrict__ d_groups, QSort qs, DtDesc dt)
{
	const int ngroups = *d_groups;
	if (!qsort_on(qs, ngroups)) return;
	const int T = ngroups * qs.chunks;
	for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T; t += gridDim.x * blockDim.x) {
		const int group = t / qs.chunks, chunk = t - group * qs.chunks;
		const ParentRec p = parents[group];
		const Rot9 R = rots[p.rot];
		const float4 c = qs.cen[chunk];
		const float h = 0.5f * p.w;
		const float q[3] = {R.r[0] * c.x + R.r[1] * c.y + R.r[2] * c.z + p.x + h - dt.xmin_f, R.r[3] * c.x + R.r[4] * c.y + R.r[5] * c.z + p.y + h - dt.ymin_f,
		                    R.r[6] * c.x + R.r[7] * c.y + R.r[8] * c.z + p.z + h - dt.zmin_f};
		unsigned key = 0;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const unsigned v = (unsigned)min(max((int)(q[k] * dt.scale_f), 0), dt.V - 1) >> qs.shift;
#pragma unroll
			for (int b = 0; b < 5; b++) key |= ((v >> b) & 1u) << (3 * b + k);
		}
		qs.keys[t] = key;
		atomicAdd(&qs.hist[key], 1u);
	}
}
__global__ void task_scatter_kernel(const int* __restrict__ d_groups, QSort qs)
{
	const int ngroups = *d_groups;
	if (!qsort_on(qs, ngroups)) return;
	const int T = ngroups * qs.chunks;
	for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T; t += gridDim.x * blockDim.x)
		qs.order[atomicAdd(&qs.hist[qs.keys[t]], 1u)] = (unsigned)t;          // order inside a bucket is arbitrary: no bound depends on it
}
// exclusive scan of the 32 768 counters by ONE workgroup: the whole histogram is staged in LDS (128 KB + padding against the 32-way bank
// conflict of "thread t owns bins 32 t .. 32 t + 31"), coalesced both ways
__global__ __launch_bounds__(1024) void task_scan_kernel(const int* __restrict__ d_groups, QSort qs)
{
	constexpr int per = kSortBins / 1024;            // 32 consecutive bins per thread
	__shared__ unsigned lds[kSortBins + kSortBins / per];
	__shared__ unsigned wtot[16];
	if (!qsort_on(qs, *d_groups)) return;
	for (int i = threadIdx.x; i < kSortBins; i += 1024) lds[i + i / per] = qs.hist[i];
	__syncthreads();
	const int b0 = threadIdx.x * (per + 1);
	unsigned local = 0;
#pragma unroll
	for (int k = 0; k < per; k++) local += lds[b0 + k];
	unsigned incl = local;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if ((int)(threadIdx.x & 63) >= o) incl += v; }
	if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
	__syncthreads();
	unsigned before = 0;
	for (int w = 0; w < (int)(threadIdx.x >> 6); w++) before += wtot[w];
	unsigned run = before + incl - local;
#pragma unroll
	for (int k = 0; k < per; k++) { const unsigned c = lds[b0 + k]; lds[b0 + k] = run; run += c; }
	__syncthreads();
	for (int i = threadIdx.x; i < kSortBins; i += 1024) qs.hist[i] = lds[i + i / per];
}
int qsort_shift(int V) { int s = 0; while (((V - 1) >> s) >= 32) s++; return s; }   // 5 bits per axis: 16-voxel cells at V = 300 and 512
size_t qsort_hist_bytes() { return sizeof(unsigned) * kSortBins; }
// orders the items of the round whose expansions bnb_queue_kernel has just listed (count on the device); a round below qs.min_groups is left alone
hipError_t launch_queue_sort(const ParentRec* parents, const Rot9* rots, const int* d_groups, int max_groups, const QSort& qs, const DtDesc& dt, hipStream_t stream)
{
	if (!qs.order || max_groups < qs.min_groups) return hipSuccess;
	// qs.hist is all zero here: cleared at allocation, and again by the bound evaluation of every round that used it (bounds_queue_kernel)
	const int blocks = (int)std::min<size_t>(((size_t)max_groups * qs.chunks + 255) / 256, 2048);
	hipLaunchKernelGGL(task_key_kernel, dim3(blocks), dim3(256), 0, stream, parents, rots, d_groups, qs, dt);
	hipLaunchKernelGGL(task_scan_kernel, dim3(1), dim3(1024), 0, stream, d_groups, qs);
	hipLaunchKernelGGL(task_scatter_kernel, dim3(blocks), dim3(256), 0, stream, d_groups, qs);
	return hipGetLastError();
}

// the four poses the chunk cost is counted at: the identity and three fixed rotations (Rodrigues vectors (0.9, -0.5, 0.3), (-0.4, 1.1, 0.8),
// (0.6, 0.7, -1.3)).  The share of a chunk in the lines is a property of the patch, not of the pose (EXPERIMENTS R9.1): four poses average it.
__constant__ float kCostRots[4][9] = {
	{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f},
	{0.84567982f, -0.449964464f, -0.286980212f, 0.0414698496f, 0.591505408f, -0.805233896f, 0.532076955f, 0.669069052f, 0.518884122f},
	{0.219921082f, -0.74321264f, 0.631877899f, 0.372148067f, 0.662668586f, 0.649904728f, -0.901743054f, 0.0922243893f, 0.422319949f},
	{0.122044131f, 0.98462534f, 0.124972485f, -0.646330416f, 0.174399301f, -0.742860556f, -0.753234506f, 0.00988825131f, 0.65767777f}};
// one thread per point, a wavefront = 64 consecutive points (chunk_pts is a multiple of 256: a wavefront lies in one chunk).  The index is the
// float fast path's without its exactness test, in separate multiply and add: a cost model, restated operation for operation by the test.
__global__ __launch_bounds__(256) void bounds_chunk_cost_kernel(const float4* __restrict__ src, int N, int chunk_pts, DtDesc dt, int* __restrict__ cost)
{
	const int i = blockIdx.x * 256 + (int)threadIdx.x, lane = (int)threadIdx.x & 63, first_pt = i - lane;
	if (first_pt >= N) return;
	const bool have = i < N;
	const float4 p = src[have ? i : N - 1];
	const unsigned V = (unsigned)dt.V;
	int lines = 0;
	for (int r = 0; r < 4; r++) {
		const float* R = kCostRots[r];
		const float rx = R[0] * p.x + R[1] * p.y + R[2] * p.z, ry = R[3] * p.x + R[4] * p.y + R[5] * p.z, rz = R[6] * p.x + R[7] * p.y + R[8] * p.z;
		const int ix = (int)((rx - dt.xmin_f) * dt.scale_f + 0.5f), iy = (int)((ry - dt.ymin_f) * dt.scale_f + 0.5f), iz = (int)((rz - dt.zmin_f) * dt.scale_f + 0.5f);
		const bool in = have && (unsigned)ix < V && (unsigned)iy < V && (unsigned)iz < V;
		// a 256-B brick is two lines: z & 2 picks the half (brick_z)
		const int line = in ? (int)((((((unsigned)iz >> 2) * (unsigned)dt.VB + ((unsigned)iy >> 2)) * (unsigned)dt.VB + ((unsigned)ix >> 2)) << 1) | (((unsigned)iz >> 1) & 1u)) : -1;
		bool first = in;
		for (int j = 0; j < 63; j++) {
			const int o = __shfl(line, j, 64);
			if (j < lane && o == line) first = false;
		}
		lines += __popcll(__ballot(first));
	}
	if (lane == 0) { const int chunk = first_pt / chunk_pts; atomicAdd(cost + chunk, lines); atomicAdd(cost + 8 + chunk, 4); }
}
// the plan of the cuts from the totals (bounds_cut_plan): what depends on the cloud and the weight only is worked out here, once
__global__ void bounds_cut_plan_kernel(int* __restrict__ cost, int a_q8)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) bounds_cut_plan(cost, a_q8, cost + kBoundsCost);
}
hipError_t launch_bounds_chunk_cost(const float4* src, int N, const DtDesc& dt, int a_q8, int* cost, hipStream_t stream)
{
	hipError_t e = hipMemsetAsync(cost, 0, kBoundsCost * sizeof(int), stream);
	if (e != hipSuccess) return e;
	if ((N + kBoundsThreads - 1) / kBoundsThreads >= 32 && dt.layout == 1 && bounds_lean(dt)) {   // else no 8-chunk shape (bounds_shape), or no pair launch: no cost, equal cuts
		int chunk_pts = (N + 7) / 8;
		chunk_pts = (chunk_pts + kBoundsThreads - 1) / kBoundsThreads * kBoundsThreads;
		hipLaunchKernelGGL(bounds_chunk_cost_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, src, N, chunk_pts, dt, cost);
	}
	hipLaunchKernelGGL(bounds_cut_plan_kernel, dim3(1), dim3(64), 0, stream, cost, a_q8);
	return hipGetLastError();
}

hipError_t bounds_xcd_stamps_take(unsigned long long* out, hipStream_t stream)
{
#ifdef GOICP_BOUNDS_XCD_STAMPS
	unsigned long long clear[kXcdStampRows * kXcdStampStride] = {}, got[kXcdStampRows * kXcdStampStride];
	for (int r = 0; r < kXcdStampRows; r++) clear[r * kXcdStampStride] = ~0ull;
	hipError_t e = hipStreamSynchronize(stream);
	if (e == hipSuccess) e = hipMemcpyFromSymbol(got, HIP_SYMBOL(g_xcd_stamps), sizeof(got));
	if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_xcd_stamps), clear, sizeof(clear));
	for (int r = 0; r < kXcdStampRows; r++)
		for (int c = 0; c < kXcdStampCols; c++) out[r * kXcdStampCols + c] = got[r * kXcdStampStride + c];
	return e;
#else
	(void)out; (void)stream;
	return hipErrorNotSupported;
#endif
}

hipError_t launch_bounds(const float4* src, int N, const DtDesc& dt, const Rot9* rots, const CubeRec* cubes, const ParentRec* parents,
                         int B, float* scratch, float* ub, float* lb, hipStream_t stream, const BoundsOrder* bo)
{
	if (B <= 0 || N <= 0) return hipSuccess;
	int groups, chunks, chunk_pts;
	bounds_shape(B, N, &groups, &chunks, &chunk_pts);
	dim3 grid(groups * chunks), block(kBoundsThreads);
	const int* alias = nullptr;                          // what this launch's finalize reads: set only behind a pre-pass that wrote it
	const int* alias_ctl = nullptr;
	if (bo && bo->mode > 0 && cubes && !parents && dt.layout == 1 && bounds_lean(dt) && groups >= bo->min_groups && bo->max_runs >= 1 && bo->max_runs <= kBoundsOrderMaxRuns) {
		const bool balanced = bo->mode == 2 && chunks == 8 && bo->balance && bo->cost;
		BoundsOrder pre = *bo;
		if (bo->mode != 2 || chunks == 1) pre.alias = nullptr;   // copies are skipped by the pair launch over several chunks only: elsewhere the table is not built
		alias = pre.alias; alias_ctl = pre.alias ? bo->ctl : nullptr;
		hipLaunchKernelGGL(bounds_order_kernel, dim3(bo->max_runs), dim3(1024), 0, stream, cubes, B, groups, dt, pre, balanced ? 1 : 0);
		if (bo->mode == 1) {
			hipLaunchKernelGGL((dt.trunc > 0.f ? bounds_ordered_kernel<true> : bounds_ordered_kernel<false>), grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups,
			                   chunks, chunk_pts, scratch, ub, lb, bo->order, bo->ctl, 1);
		} else {
			const int max_items = (int)bounds_order_items(groups, bo->max_runs);
			const int nblocks = chunks == 8 ? 8 * bounds_pair_slots(max_items, balanced) : max_items * chunks;
			hipLaunchKernelGGL((dt.trunc > 0.f ? bounds_pair_kernel<true> : bounds_pair_kernel<false>), dim3(nblocks), block, 0, stream, src, N, dt, rots, cubes, parents,
			                   B, groups, max_items, chunks, chunk_pts, scratch, ub, lb, bo->pairs, bo->ctl, alias);
		}
	} else
	if (dt.trunc > 0.f) {                                                // the truncated objective (DtDesc::trunc): the same four choices
		if (dt.layout == 0)
			hipLaunchKernelGGL((bounds_kernel<0, false, true>), grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub, lb);
		else if (dt.layout == 1 && bounds_lean(dt))
			hipLaunchKernelGGL((bounds_kernel<1, true, true>), grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub, lb);
		else if (dt.layout == 1)
			hipLaunchKernelGGL((bounds_kernel<1, false, true>), grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub, lb);
		else
			hipLaunchKernelGGL((bounds_kernel<2, false, true>), grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub, lb);
	} else
	if (dt.layout == 0)
		hipLaunchKernelGGL(bounds_kernel<0>, grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub, lb);
	else if (dt.layout == 1 && bounds_lean(dt))
		hipLaunchKernelGGL((bounds_kernel<1, true>), grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub, lb);
	else if (dt.layout == 1)
		hipLaunchKernelGGL(bounds_kernel<1>, grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub, lb);
	else
		hipLaunchKernelGGL(bounds_kernel<2>, grid, block, 0, stream, src, N, dt, rots, cubes, parents, B, groups, chunks, chunk_pts, scratch, ub, lb);
	if (chunks > 1) {
		int t = groups * 2 * kGroup;
		hipLaunchKernelGGL(bounds_finalize, dim3((t + 255) / 256), dim3(256), 0, stream, scratch, B, groups, chunks, ub, lb, alias, alias_ctl);
	}
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// (b) ICP: exact 1-NN in the flattened k-d tree -- 64-ary, four queries per WAVEFRONT.
// Measured on MI355X, a per-lane walk of a binary tree is hopeless at this size: 30 k queries are
// only 475 wavefronts, every step is a dependent, divergent access, and a wave is as slow as its
// unluckiest lane (1.3 ms per pass, 3.9 ms for queries far from the surface).  So the tree the
// host builds by median splits is flattened into a 64-ary hierarchy of tight bounding boxes, walked
// cooperatively:
//   * a wavefront is four 16-lane rows; a row owns one query, each of its lanes four of the 64
//     child boxes of the current group (six float4 loads per lane), and a leaf's 16 slots map onto
//     the row's 16 lanes;
//   * minima inside a row are DPP butterflies (quad_perm, row_half_mirror, row_mirror) -- no scalar
//     loops, no LDS, no per-lane stack; "any lane of my row" is a slice of a ballot;
//   * a child is one sortable key (distance bits | sub-index); children are TAKEN in ascending key
//     order, so "next key above the best distance" means the group is exhausted -- no pending masks,
//     no re-filtering; the two nearest remaining leaves are scanned per step (two loads in flight,
//     one wait);
//   * the search starts from the upper bound (|q - centre(v)| + DT[v] + 0.9 voxel)^2 read from the
//     distance transform the engine already holds, so queries far from the surface prune as
//     well as near ones; the nearest child of the root is fetched together with that seed;
//   * rows are at different stages of their walks, so one loop iteration runs (at most) the two
//     step kinds "enter a group" and "scan leaves" under the rows' exec masks.
// History (bunny, 30 379 queries, converged pose, per pass): per-lane binary walk 1300 us; one
// wavefront per query with ballot/readlane loops 42 us (instruction-issue bound, ~1250
// wave-instructions per query); this kernel 26 us (~440 per query; what is left is the chain of
// dependent memory round trips of the slowest wavefront).
// The binary depth follows the cloud (full leaves, sparse root group, kdtree.cpp): K = 2 box levels up to
// 65 536 target points, K = 3 up to 4.2 M.
// Exactness: box lower bounds use the same monotone float accumulation as the point distances and
// the boxes are exact, ties go to the lowest original index -> identical to a brute-force scan.
// ------------------------------------------------------------------------------------------------
#ifndef GOICP_ICP_THREADS
#define GOICP_ICP_THREADS 256
#endif
// up to this many source points the pass deals strangers, not neighbours, to a wavefront (icp_pass_kernel).  Measured, iterations/s
// neighbours | strangers: bunny 30 k 26.7 k | 29.0 k; synthetic 40 k 16.4 k | 16.5 k; 100 k 8.6 k | 7.5 k; spanner 150 k 12.6 k | 11.7 k;
// 250 k 4.2 k | 3.3 k; 500 k 2.06 k | 1.45 k
// (kIcpStridedMaxN lives in device.hpp: the engine sizes the accumulators by it)
constexpr int kIcpThreads = GOICP_ICP_THREADS;     // 4 wavefronts = 16 queries per workgroup

// Upper bound on the NN distance from the distance transform.  For ANY voxel v:
//   d(q, NN) <= |q - centre(v)| + DT[v] + sqrt(3)/2 voxel
// (DT[v] is the exact distance from v's centre to the centre of the nearest seed voxel, and a target
// point lies within sqrt(3)/2 voxel of the centre of the voxel it seeded).  v = the grid voxel nearest
// to q (clamped into the grid, so queries outside it are covered too); |q - centre(v)| is computed
// explicitly, so neither the reference's index rounding nor its out-of-grid extension matters here.
// 0.9 voxel + 1e-5 relative cover sqrt(3)/2 = 0.866 and the float rounding of this expression.
template <int LAYOUT>
__device__ __forceinline__ float nn_upper_bound(const DtDesc& dt, float qx, float qy, float qz)
{
	const float inv = 1.0f / dt.scale_f;
	const int V1 = dt.V - 1;
	const int ix = min(max((int)rintf((qx - dt.xmin_f) * dt.scale_f), 0), V1);
	const int iy = min(max((int)rintf((qy - dt.ymin_f) * dt.scale_f), 0), V1);
	const int iz = min(max((int)rintf((qz - dt.zmin_f) * dt.scale_f), 0), V1);
	const float cx = dt.xmin_f + (float)ix * inv, cy = dt.ymin_f + (float)iy * inv, cz = dt.zmin_f + (float)iz * inv;
	const float ex = qx - cx, ey = qy - cy, ez = qz - cz;
	const float d = (__fsqrt_rn(ex * ex + ey * ey + ez * ez) + dt_fetch<LAYOUT>(dt, ix, iy, iz) + 0.9f * inv) * 1.00001f;
	return d * d;
}

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v)
{
	return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ unsigned row_min_u32(unsigned v)      // min over the lane's 16-lane row, in every lane
{
	v = min(v, dpp_u32<0xB1>(v));     // quad_perm [1,0,3,2]
	v = min(v, dpp_u32<0x4E>(v));     // quad_perm [2,3,0,1]
	v = min(v, dpp_u32<0x141>(v));    // row_half_mirror
	v = min(v, dpp_u32<0x140>(v));    // row_mirror
	return v;
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_sum_f32(float v)            // sum over the lane's 16-lane row, in every lane
{
	v += dpp_f32<0xB1>(v);
	v += dpp_f32<0x4E>(v);
	v += dpp_f32<0x141>(v);
	v += dpp_f32<0x140>(v);
	return v;
}

struct Box6x4 { float4 lox, loy, loz, hix, hiy, hiz; };   // the four children 4l..4l+3 of a lane
__device__ __forceinline__ Box6x4 load_child_boxes4(const float* __restrict__ g, int l)
{
	const float4* r = reinterpret_cast<const float4*>(g);
	return Box6x4{r[l], r[16 + l], r[32 + l], r[48 + l], r[64 + l], r[80 + l]};
}
__device__ __forceinline__ float box_lb1(float lox, float loy, float loz, float hix, float hiy, float hiz, float qx, float qy, float qz)
{
	const float ex = fmaxf(fmaxf(lox - qx, qx - hix), 0.f);
	const float ey = fmaxf(fmaxf(loy - qy, qy - hiy), 0.f);
	const float ez = fmaxf(fmaxf(loz - qz, qz - hiz), 0.f);
	float d = ex * ex;
	d += ey * ey;
	d += ez * ez;
	return d;
}
__device__ __forceinline__ void boxes_lb4(const Box6x4& b, float qx, float qy, float qz, float lb[4])
{
	lb[0] = box_lb1(b.lox.x, b.loy.x, b.loz.x, b.hix.x, b.hiy.x, b.hiz.x, qx, qy, qz);
	lb[1] = box_lb1(b.lox.y, b.loy.y, b.loz.y, b.hix.y, b.hiy.y, b.hiz.y, qx, qy, qz);
	lb[2] = box_lb1(b.lox.z, b.loy.z, b.loz.z, b.hix.z, b.hiy.z, b.hiz.z, qx, qy, qz);
	lb[3] = box_lb1(b.lox.w, b.loy.w, b.loz.w, b.hix.w, b.hiy.w, b.hiz.w, qx, qy, qz);
}
// A child is held as one sortable key: the bits of its box distance (>= 0, so they order like the
// float) with the two low mantissa bits replaced by the child's sub-index 0..3; 0xffffffff once taken.
// Pruning with (key & ~3) <= bits(best) is conservative by at most those two bits (a child that could
// just have been skipped is visited): exactness is untouched.
__device__ __forceinline__ void boxes_keys4(const Box6x4& b, float qx, float qy, float qz, unsigned key[4])
{
	float lb[4];
	boxes_lb4(b, qx, qy, qz, lb);
#pragma unroll
	for (int j = 0; j < 4; j++) key[j] = (__float_as_uint(lb[j]) & ~3u) | (unsigned)j;
}
// Take the nearest remaining child of the row: returns its key (uniform in the row; 0xffffffff when
// none is left) and the child 0..63; the owner lane marks it taken.  Because children are taken in
// ascending order, "key above the best distance" means the whole group is exhausted: no pending
// masks, no re-filtering.
__device__ __forceinline__ unsigned row_take(unsigned key[4], int l, int row, int& child)
{
	const unsigned mine = min(min(key[0], key[1]), min(key[2], key[3]));
	const unsigned m = row_min_u32(mine);
	const unsigned owners = (unsigned)(__ballot(mine == m) >> (16 * row)) & 0xffffu;
	const int wl = __ffs((int)owners) - 1;
	const unsigned j = m & 3u;
	if (l == wl) {
		key[0] = j == 0u ? 0xffffffffu : key[0];
		key[1] = j == 1u ? 0xffffffffu : key[1];
		key[2] = j == 2u ? 0xffffffffu : key[2];
		key[3] = j == 3u ? 0xffffffffu : key[3];
	}
	child = 4 * wl + (int)j;
	return m;
}

// Exact 1-NN of the row's query.  `active` rows walk; the others idle through the loop.  On return
// best/idx are uniform in the row and exactly one lane of an active row has `mine` set: the one whose
// leaf slot holds the neighbour (its coordinates and slot ride along in that lane).
//
// TWO: also return best2, a lower bound on the squared distance from the query to EVERY target point other than the
// neighbour (the walk then prunes with the second-best distance; the DT seed takes part as a pseudo-candidate, which can
// only make best2 smaller, i.e. more conservative).  The ICP pass caches (query position, neighbour, sqrt(best2)) per
// source point: on a later pass at position q' the cached point m is still THE nearest neighbour whenever
// |q' - m| + |q' - q_ref| < sqrt(best2_ref) -- every other point is at least sqrt(best2_ref) - |q' - q_ref| away -- so the
// walk is skipped exactly, not approximately.
//
// CAP (the gated ICP pass): the pruning bound starts at min(seed distance, cap) -- a box whose key lies above cap's bits is never entered,
// and a query whose seed lies beyond the cap and that has no box within it ends at its first step.  The cap is non-strict, so every
// target point with d^2 <= cap is still found, with the same neighbour and tie rule (a point AT the cap beats the empty candidate
// INT_MAX); a query with nothing inside the cap returns best = cap with NO lane `mine`: its neighbour is unspecified and the caller
// must not use it.  cap = +inf is the uncapped walk.
struct RowNn { float best; int idx; bool mine; float mx, my, mz; int slot; float best2; };

template <int K, int LAYOUT, bool TWO = false, int LEAVES = 2, bool CAP = false>
__device__ __forceinline__ RowNn rows_nearest(const KdDesc& kd, const DtDesc& dt, const Box6x4& rootb, int l, int row,
                                              float qx, float qy, float qz, bool active, float cap = 0.f)
{
	static_assert(!CAP || !TWO, "the capped walk has no second-best form");
	// no row of this wavefront needs a walk (every query hit the neighbour cache): nothing to fetch, nothing to compute
	if (!__any(active)) return RowNn{INFINITY, INT_MAX, false, 0.f, 0.f, 0.f, 0, INFINITY};
	unsigned key[K][4];
	int node[K];                              // group index at each level; leaves of level K-1 are node*64 + c
	node[0] = 0;
	boxes_keys4(rootb, qx, qy, qz, key[0]);
#pragma unroll
	for (int L = 1; L < K; L++) {
		node[L] = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) key[L][j] = 0xffffffffu;
	}
	// The child of the root with the smallest box distance survives any valid bound (the true
	// neighbour's child has lb <= d_nn), so its boxes are fetched together with the DT seed instead
	// of after it: one dependent memory round trip less.
	Box6x4 fb = rootb;
	if constexpr (K > 1) {
		row_take(key[0], l, row, node[1]);
		fb = load_child_boxes4(kd.boxes[1] + (size_t)node[1] * 384, l);
	}
	RowNn r{0.f, INT_MAX, false, 0.f, 0.f, 0.f, 0, INFINITY};
	if (!TWO && dt.nn_ids) {
		// the walk starts from a REAL candidate: a target point whose seed voxel is nearest to the query's voxel (clamped into
		// the grid) -- nearly always the neighbour itself, so every box beyond the true distance is pruned from the first step
		// (the distance-transform bound below carries up to 1.8 voxels of slack: far from the surface that is a shell with
		// dozens of leaves in it, and the pass lasts as long as its longest walk).  Any target point is a valid candidate, so
		// exactness does not depend on the table; lane 0 of the row holds it until a scan finds a nearer one (or an equally
		// near one with a lower index).
		const int V1 = dt.V - 1;
		const int ix = min(max((int)rintf((qx - dt.xmin_f) * dt.scale_f), 0), V1);
		const int iy = min(max((int)rintf((qy - dt.ymin_f) * dt.scale_f), 0), V1);
		const int iz = min(max((int)rintf((qz - dt.zmin_f) * dt.scale_f), 0), V1);
		size_t off;
		if (LAYOUT == 0) off = ((size_t)iz * dt.V + iy) * dt.V + ix;
		else off = brick_index(ix, iy, iz, dt.VB);
		const int slot = dt.nn_ids[off];
		const float4 pt = kd.pts[slot];
		const float d0 = qx - pt.x, d1 = qy - pt.y, d2 = qz - pt.z;
		float e = d0 * d0;                                                 // the leaf scan's accumulation order: the same bits
		e += d1 * d1;
		e += d2 * d2;
		r.best = e; r.idx = __float_as_int(pt.w); r.mine = l == 0; r.mx = pt.x; r.my = pt.y; r.mz = pt.z; r.slot = slot;
	} else
		r.best = nn_upper_bound<LAYOUT>(dt, qx, qy, qz);
	if constexpr (CAP) {
		if (r.best > cap) { r.best = cap; r.idx = INT_MAX; r.mine = false; }
	}
	unsigned bbits = __float_as_uint(r.best);
	unsigned b2bits = 0x7f800000u;                // +inf: nothing but the neighbour seen yet
	int d = 0;
	if constexpr (K > 1) {
		boxes_keys4(fb, qx, qy, qz, key[1]);
		d = 1;
	}
	bool done = !active;
	while (__any(!done)) {
		// One step per row and iteration: leave exhausted levels (cascading through the unrolled
		// blocks below), then either enter the nearest child group or scan the two nearest leaves.
		bool acted = done;
#pragma unroll
		for (int L = K - 1; L >= 0; L--) {
			if (!acted && d == L) {
				int c;
				const unsigned m = row_take(key[L], l, row, c);
				// bbits / b2bits are the bits of a distance, finite or +inf (<= 0x7f800000), in every template form and from the first step
				// on, so the all-taken key 0xffffffff always lies above them: an emptied group is left here without a test of its own
				// (rows_knn's bound is 0xffffffff while its list is short, and it has one)
				if ((m & ~3u) > (TWO ? b2bits : bbits)) {            // nothing left within the best (TWO: second-best) distance
					if (L == 0) { done = true; acted = true; }
					else d = L - 1;
				} else if (L == K - 1 && LEAVES == 4 && !TWO) {
					// ---- scan the FOUR nearest remaining leaves of the group: four loads in flight, one wait.  A pass at
					// bunny scale lasts as long as its longest walk (a handful of far-from-surface queries with dozens of
					// near-equidistant leaves; every step is a dependent round trip), so halving the steps of a walk is worth
					// the extra row_takes; leaves beyond the bound re-read the first one and are ignored ----
					const int s0 = (node[L] * 64 + c) * kLeafSlots + l;
					int sl[4] = {s0, s0, s0, s0};
					bool use[4] = {true, false, false, false};
#pragma unroll
					for (int j = 1; j < 4; j++) {
						int cj;
						const unsigned mj = row_take(key[L], l, row, cj);
						use[j] = (mj & ~3u) <= bbits;
						if (use[j]) sl[j] = (node[L] * 64 + cj) * kLeafSlots + l;
					}
					float4 pq[4];
#pragma unroll
					for (int j = 0; j < 4; j++) pq[j] = kd.pts[sl[j]];
					float4 pt = pq[0];
					int sb = sl[0];
					float e;
					{
						const float d0 = qx - pt.x, d1 = qy - pt.y, d2 = qz - pt.z;
						e = d0 * d0;                                     // L2_Simple_Adaptor accumulation order
						e += d1 * d1;
						e += d2 * d2;
					}
#pragma unroll
					for (int j = 1; j < 4; j++) {
						const float d0 = qx - pq[j].x, d1 = qy - pq[j].y, d2 = qz - pq[j].z;
						float dj = d0 * d0;
						dj += d1 * d1;
						dj += d2 * d2;
						const bool wins = use[j] && (dj < e || (dj == e && __float_as_int(pq[j].w) < __float_as_int(pt.w)));
						if (wins) { pt = pq[j]; e = dj; sb = sl[j]; }
					}
					const unsigned db = __float_as_uint(e);
					const unsigned dmin = row_min_u32(db);
					const unsigned id = (unsigned)__float_as_int(pt.w);
					const unsigned idmin = row_min_u32(db == dmin ? id : 0x7fffffffu);   // ties -> lowest original index
					if (dmin < bbits || (dmin == bbits && (int)idmin < r.idx)) {
						bbits = dmin;
						r.idx = (int)idmin;
						r.mine = db == dmin && id == idmin;
						r.mx = pt.x; r.my = pt.y; r.mz = pt.z; r.slot = sb;
					}
					acted = true;
				} else if (L == K - 1) {
					// ---- scan the two nearest remaining leaves of the group: one slot per lane each ----
					int c2;
					const unsigned m2 = row_take(key[L], l, row, c2);
					const int sa = (node[L] * 64 + c) * kLeafSlots + l;
					const bool dup = (m2 & ~3u) > (TWO ? b2bits : bbits);   // no second leaf worth scanning: the first one twice
					int sb = (node[L] * 64 + (dup ? c : c2)) * kLeafSlots + l;
					const float4 pa = kd.pts[sa];
					float4 pt = kd.pts[sb];
					const float d0 = qx - pa.x, d1 = qy - pa.y, d2 = qz - pa.z;
					float da = d0 * d0;                              // L2_Simple_Adaptor accumulation order
					da += d1 * d1;
					da += d2 * d2;
					const float e0 = qx - pt.x, e1 = qy - pt.y, e2 = qz - pt.z;
					float e = e0 * e0;
					e += e1 * e1;
					e += e2 * e2;
					const bool a_wins = da < e || (da == e && __float_as_int(pa.w) < __float_as_int(pt.w));
					const float other = dup ? INFINITY : (a_wins ? e : da);   // this lane's second candidate (TWO)
					if (a_wins) { pt = pa; e = da; sb = sa; }
					const unsigned db = __float_as_uint(e);
					const unsigned dmin = row_min_u32(db);
					const unsigned id = (unsigned)__float_as_int(pt.w);
					const unsigned idmin = row_min_u32(db == dmin ? id : 0x7fffffffu);   // ties -> lowest original index
					if constexpr (TWO) {
						// the two smallest of {best, best2, this scan's candidates}: the scan's runner-up is the row minimum with
						// the winning lane represented by its other candidate
						const unsigned second = row_min_u32((db == dmin && id == idmin) ? __float_as_uint(other) : db);
						b2bits = min(max(bbits, dmin), min(b2bits, second));
					}
					if (dmin < bbits || (dmin == bbits && (int)idmin < r.idx)) {
						bbits = dmin;
						r.idx = (int)idmin;
						r.mine = db == dmin && id == idmin;
						r.mx = pt.x; r.my = pt.y; r.mz = pt.z; r.slot = sb;
					}
					acted = true;
				} else {
					// ---- enter the nearest remaining child group one level down ----
					const int NL = L + 1 < K ? L + 1 : L;
					node[NL] = node[L] * 64 + c;
					const Box6x4 cb = load_child_boxes4(kd.boxes[NL] + (size_t)node[NL] * 384, l);
					boxes_keys4(cb, qx, qy, qz, key[NL]);
					d = NL;
					acted = true;
				}
			}
		}
	}
	r.best = __uint_as_float(bbits);
	r.best2 = __uint_as_float(b2bits);
	return r;
}

// Workgroup-shared state of one ICP iteration: the per-wavefront sums of the pass and the finalize's scratch, in ONE
// __shared__ object (a second one beside it can make the compiler drain the memory pipeline before LDS reads).
constexpr int kFinThreads = 1024;                  // the stand-alone finalize: 256 row streams x four float4 columns
struct FinScratch { double wsum[kFinThreads / 64][kIcpAcc]; double sums[kIcpAcc]; float red[kIcpThreads / 16][kIcpAcc]; int last; IcpState st; };   // red: one row of sums per 16-lane row
template <int T> __device__ __forceinline__ void finalize_reduce(const float* __restrict__ partials, int nblocks, FinScratch& sh);
template <bool GATE = false, bool ROBUST = false>
__device__ __forceinline__ void finalize_rows(const double* __restrict__ sums, IcpState* __restrict__ state, const IcpState& rd, int lane);

// Robust-kernel ICP (goicp_set_icp_robust): the weight w of a correspondence from its residual r (metric 0: the distance d = sqrtf(d^2); metric 1:
// |(q - m) . n|) and its term rho of the robust cost C from the distance d, with u = r / c, v = d / c.  Float, on the owning lane, operation by
// operation as written (-ffp-contract=off; `/` and __fsqrt_rn are the correctly rounded ones), so that a twin can restate them:
//   1 Huber          w = 1 if r <= c else c / r         rho = d^2 if d <= c else 2 c d - c^2
//   2 Cauchy         w = 1 / (1 + u^2)                  rho = c^2 log1pf(v^2)
//   3 Geman-McClure  w = 1 / (1 + u^2)^2                rho = d^2 / (1 + v^2)
//   4 Tukey          w = (1 - u^2)^2 if r <= c else 0   rho = c^2/3 v^2 (3 - 3 v^2 + v^4) [= c^2/3 (1 - (1 - v^2)^3), without the cancellation] if d <= c else c^2/3
// rho <= d^2 for every kernel; the min() holds that against rounding (and against an overflowing v^2), so C <= sum d^2 and the pass's fixed-point
// scale serves.  rho is only read by the stop test.  A Huber term inside the scale is w = 1.0f, rho = the walk's d^2 bits: the plain pass, bit for bit.
struct RobustTerms { float w, rho; };
__device__ __forceinline__ RobustTerms robust_terms(int rk, float c, float r, float d, float d2)
{
	RobustTerms o;
	const float u = r / c, u2 = u * u;
	const float v = d / c, v2 = v * v;
	const float c2 = c * c;
	if (rk == 1) {
		o.w = r <= c ? 1.f : c / r;
		o.rho = d <= c ? d2 : 2.f * c * d - c2;
	} else if (rk == 2) {
		o.w = 1.f / (1.f + u2);
		o.rho = c2 * log1pf(v2);
	} else if (rk == 3) {
		const float s1 = 1.f + u2;
		o.w = 1.f / (s1 * s1);
		o.rho = d2 / (1.f + v2);
	} else {
		const float a1 = 1.f - u2;
		o.w = r <= c ? a1 * a1 : 0.f;
		o.rho = d <= c ? (c2 / 3.f) * (v2 * (3.f - 3.f * v2 + v2 * v2)) : c2 / 3.f;
	}
	o.rho = fminf(o.rho, d2);
	return o;
}

// FUSED: the workgroup that arrives last (one ticket per launch; agent-scope release before the ticket, acquire
// after it -- cdna_hip_programming.md Guideline 16, counter form) also runs the finalize, so an ICP iteration is ONE
// launch.  `ticket` is zero between launches: zeroed when the engine is created, reset by the last arriver.
// nn_cache (two float4 per source point: {q_ref.xyz, sqrt(best2_ref)}, {neighbour xyz, its original index}) != nullptr:
// the exact skip test of rows_nearest<TWO>'s comment; entries never go stale (they are statements about the static
// target cloud), an entry with sqrt(best2_ref) = 0 (fresh engine, tied neighbours) always walks.
// SLICE (ACC form only, goicp_icp_run_collective): the launch covers workgroups [b0, b0 + gridDim.x) of the world-1 grid -- the
// global workgroup index blockIdx.x + b0 picks the queries and the replica, so every workgroup forms the same float row sums from the
// same 16 queries as in a full pass, and the integer totals of the slices of all ranks add up to the world-1 totals bit for bit.
// The body is shared with icp_opt_pass_kernel (the opt-in iterations), which in a batch runs the ACC form on one pose slot per blockIdx.y.  Its pointers carry no
// __restrict__ of their own: they come from the kernels' restrict parameters, which keeps icp_pass_kernel's code what it was before the split.
// GATE (goicp_set_icp_gate; ACC form only): the owning lane zeroes its terms when d^2 > IcpState::g2 and contributes 1 to a count otherwise; the
// accumulator block then has the plane pass's stride (kIcpPlaneStride words per replica), the count a plain integer in word 16.  `capped`: the walk
// prunes at g2 (rows_nearest<CAP>); an outlier's row may then have no owning lane at all.
// ROBUST (goicp_set_icp_robust; ACC form only, the plain walk): the owning lane multiplies its 15 Kabsch terms by robust_terms' weight -- d^2 stays
// unweighted: err is over all N points -- and hands w and rho to two more column sums; the block has the plane pass's stride, W = sum w in word 16
// (scaled by kIcpRobustWScale), C = sum rho in word 17 (scaled as the terms).
template <int K, int LAYOUT, bool FUSED, bool CACHE, int LEAVES, bool STRIDED, bool ACC, bool SLICE, bool GATE = false, bool ROBUST = false>
__device__ __forceinline__ void icp_pass_body(const float4* src, int N, IcpState* st, const KdDesc& kd, const DtDesc& dt, float* partials, int* ticket,
                                              float4* nn_cache, int* hit_counter, int b0, int capped = 0)
{
	static_assert(!SLICE || (ACC && !FUSED), "a slice of the pass exists in the fixed-point form only");
	static_assert(!GATE || (ACC && !FUSED && !CACHE && !SLICE), "the gated pass exists in the fixed-point form only; every query walks");
	static_assert(!ROBUST || (ACC && !FUSED && !CACHE && !SLICE && !GATE), "the robust pass exists in the fixed-point form only; every query walks; no gate");
	const int gb = SLICE ? (int)blockIdx.x + b0 : (int)blockIdx.x;   // workgroup index in the world-1 grid
	__shared__ FinScratch sh;
	float (*red)[kIcpAcc] = sh.red;                                   // [16 rows of the workgroup][16 sums]
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane >> 4, l = lane & 15;
	// Which four queries a wavefront walks.  Neighbours in the k-d order (large clouds: their walks touch the same boxes
	// and leaves, and at 1 M points the pass is throughput-bound: 926 vs 583 iterations/s) -- or, STRIDED, four queries a
	// quarter of the cloud apart (small clouds: the pass lasts as long as its slowest wavefront; far-from-surface queries
	// come in neighbourhoods, so with neighbours in one wavefront all four rows walk long and in different stages, with
	// strangers the one long walk of a wavefront runs alone: bunny 27.3 k -> 29.7 k iterations/s)
	const int nw = (N + 3) >> 2, wv = gb * (kIcpThreads / 64) + wave;
	const int i = STRIDED ? wv + row * nw : wv * 4 + row;
	const bool valid = wv < nw && i < N;
	const Box6x4 rootb = load_child_boxes4(kd.boxes[0], l);      // issued before the flag is tested: one round trip less
	const int ic = valid ? i : N - 1;
	const float4 p = src[ic];
	float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0;
	if constexpr (CACHE) { c0 = nn_cache[2 * (size_t)ic]; c1 = nn_cache[2 * (size_t)ic + 1]; }   // same round trip as p
	if (st->converged) return;                                   // loop already finished: queued launches drain
	// jly_icp3d.hpp:222-224, left-to-right float sums
	const float qx = st->R[0] * p.x + st->R[1] * p.y + st->R[2] * p.z + st->t[0];
	const float qy = st->R[3] * p.x + st->R[4] * p.y + st->R[5] * p.z + st->t[1];
	const float qz = st->R[6] * p.x + st->R[7] * p.y + st->R[8] * p.z + st->t[2];
	RowNn r;
	if constexpr (CACHE) {
		// exact skip test: the cached point is THE neighbour at q if |q - m| + |q - q_ref| < sqrt(best2_ref); a relative
		// 1e-5 and an absolute 1e-7 cover the rounding of the three square roots and sums (a failed test only costs a walk)
		const float e0 = qx - c1.x, e1 = qy - c1.y, e2 = qz - c1.z;
		float e = e0 * e0;                                       // the leaf scan's accumulation order: the same bits
		e += e1 * e1;
		e += e2 * e2;
		const float g0 = qx - c0.x, g1 = qy - c0.y, g2 = qz - c0.z;
		const float moved = __fsqrt_rn(g0 * g0 + g1 * g1 + g2 * g2);
		const bool hit = valid && (__fsqrt_rn(e) + moved) * 1.00001f + 1e-7f < c0.w;
		r = rows_nearest<K, LAYOUT, true>(kd, dt, rootb, l, row, qx, qy, qz, valid && !hit);
		if (hit_counter && hit && l == 0) atomicAdd(hit_counter, 1);      // diagnostics only (goicp_debug_cache_hits)
		if (hit) {
			r.best = e; r.idx = __float_as_int(c1.w); r.mine = l == 0; r.mx = c1.x; r.my = c1.y; r.mz = c1.z;
		} else if (valid && r.mine) {
			// the walk's result becomes the entry: position, neighbour, and what everything else is at least away
			nn_cache[2 * (size_t)i] = make_float4(qx, qy, qz, __fsqrt_rn(r.best2) * 0.99999f);
			nn_cache[2 * (size_t)i + 1] = make_float4(r.mx, r.my, r.mz, __int_as_float(r.idx));
		}
	} else if constexpr (GATE) {
		r = rows_nearest<K, LAYOUT, false, LEAVES, true>(kd, dt, rootb, l, row, qx, qy, qz, valid, capped ? st->g2 : INFINITY);
	} else {
		r = rows_nearest<K, LAYOUT, false, LEAVES>(kd, dt, rootb, l, row, qx, qy, qz, valid);
	}
	float acc[kIcpAcc];
#pragma unroll
	for (int k = 0; k < kIcpAcc; k++) acc[k] = 0.f;
	bool inlier = valid && r.mine;                               // exactly one lane of the row (GATE: at most one)
	[[maybe_unused]] RobustTerms rob{0.f, 0.f};                  // ROBUST: a row without a query adds no weight and no cost
	if constexpr (GATE) inlier = inlier && r.best <= st->g2;
	if (inlier) {
		const float ax = qx - st->cq[0], ay = qy - st->cq[1], az = qz - st->cq[2];   // pivots keep the covariance sums well conditioned
		const float bx = r.mx - st->cm[0], by = r.my - st->cm[1], bz = r.mz - st->cm[2];
		acc[0] = ax; acc[1] = ay; acc[2] = az;
		acc[3] = bx; acc[4] = by; acc[5] = bz;
		acc[6] = ax * bx; acc[7] = ax * by; acc[8] = ax * bz;
		acc[9] = ay * bx; acc[10] = ay * by; acc[11] = ay * bz;
		acc[12] = az * bx; acc[13] = az * by; acc[14] = az * bz;
		acc[15] = r.best;
		if constexpr (ROBUST) {
			const float d = __fsqrt_rn(r.best);
			rob = robust_terms(st->rk, st->rc, d, d, r.best);
#pragma unroll
			for (int k = 0; k < 15; k++) acc[k] *= rob.w;
		}
	}
	// Exactly one lane of a row holds its correspondence (the others hold zeros), so there is nothing to reduce inside a
	// row: that lane stores its 16 terms to LDS (four 16-byte stores), rows without a query store zeros, and 16 threads add
	// the workgroup's 16 rows in fixed order.  (The previous form ran 16 DPP row sums + 32 cross-row shuffles per wavefront:
	// 160 of the ~1 180 VALU instructions of a wavefront, on a kernel the counters show to be VALU-issue-limited.)
	__shared__ int gate_cnt[GATE ? kIcpThreads / 16 : 1];        // GATE: one inlier flag per row
	__shared__ float rob_red[ROBUST ? kIcpThreads / 16 : 1][2];  // ROBUST: w and rho per row
	{
		const int wrow = wave * 4 + row;
		bool owner = valid ? r.mine : l == 0;
		if constexpr (GATE) {
			// a capped walk that found nothing inside the gate leaves the row without an owning lane: its lane 0 stores the zeros
			const unsigned mine_row = (unsigned)(__ballot(valid && r.mine) >> (16 * row)) & 0xffffu;
			owner = mine_row ? (valid && r.mine) : l == 0;
		}
		if (owner) {
			float4* dst = reinterpret_cast<float4*>(red[wrow]);
			dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
			dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
			dst[2] = make_float4(acc[8], acc[9], acc[10], acc[11]);
			dst[3] = make_float4(acc[12], acc[13], acc[14], acc[15]);
			if constexpr (GATE) gate_cnt[wrow] = inlier ? 1 : 0;
			if constexpr (ROBUST) *reinterpret_cast<float2*>(rob_red[wrow]) = make_float2(rob.w, rob.rho);
		}
	}
	__syncthreads();
	if constexpr (ROBUST) {
		if (threadIdx.x >= kIcpAcc && threadIdx.x < kIcpAcc + 2) {   // W and C: float column sums in fixed order, as the 16 terms
			const int col = threadIdx.x - kIcpAcc;
			float sum = rob_red[0][col];
#pragma unroll
			for (int x = 1; x < kIcpThreads / 16; x++) sum += rob_red[x][col];
			const long long v = __double2ll_rn((double)sum * (col == 0 ? kIcpRobustWScale : (double)st->acc_scale));
			unsigned long long* a = reinterpret_cast<unsigned long long*>(partials) + (size_t)(gb & (kIcpAccReplicas - 1)) * kIcpPlaneStride + threadIdx.x;
			__hip_atomic_fetch_add(a, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	if constexpr (GATE) {
		if (threadIdx.x == kIcpAcc) {                             // the workgroup's inlier count: a plain integer, word 16 of the replica
			int c = 0;
#pragma unroll
			for (int x = 0; x < kIcpThreads / 16; x++) c += gate_cnt[x];
			unsigned long long* a = reinterpret_cast<unsigned long long*>(partials) + (size_t)(gb & (kIcpAccReplicas - 1)) * kIcpPlaneStride + kIcpAcc;
			__hip_atomic_fetch_add(a, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	if (threadIdx.x < kIcpAcc) {
		float sum = red[0][threadIdx.x];
#pragma unroll
		for (int x = 1; x < kIcpThreads / 16; x++) sum += red[x][threadIdx.x];
		if constexpr (FUSED) {
			// publish the row WRITE-THROUGH (agent-scope relaxed 8-byte stores = sc1): no release fence, i.e. no L2
			// write-back per workgroup (measured: with a release fence in each of the 1 899 workgroups the pass took 61 us
			// instead of 27)
			const float nb = __shfl_down(sum, 1, 64);
			if ((threadIdx.x & 1) == 0) {
				const unsigned long long pk = (unsigned long long)__float_as_uint(sum) | ((unsigned long long)__float_as_uint(nb) << 32);
				__hip_atomic_store(reinterpret_cast<unsigned long long*>(partials + (size_t)blockIdx.x * kIcpAcc + threadIdx.x), pk, __ATOMIC_RELAXED,
				                   __HIP_MEMORY_SCOPE_AGENT);
			}
		} else if constexpr (ACC) {
			// no row of partial sums per workgroup (on the bunny the finalize spent 4.2 of its 9.4 us fetching and adding
			// 1 899 of them) but 16 device-scope 64-bit integer adds of the sums in fixed point -- integer addition is
			// associative, so the totals are exact and independent of the arrival order: still bit-reproducible
			const long long v = __double2ll_rn((double)sum * (double)st->acc_scale);
			unsigned long long* a = reinterpret_cast<unsigned long long*>(partials) + (size_t)(gb & (kIcpAccReplicas - 1)) * (GATE || ROBUST ? kIcpPlaneStride : kIcpAcc) + threadIdx.x;
			__hip_atomic_fetch_add(a, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		} else {
			partials[(size_t)blockIdx.x * kIcpAcc + threadIdx.x] = sum;
		}
	}
	if constexpr (FUSED) {
		// the storing wave drains its stores, workgroup barrier, then ONE lane draws the ticket
		__asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
		if (threadIdx.x == 0) {
			const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			const int last = t == (int)gridDim.x - 1;
			if (last) {
				__hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // next launch starts from zero
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
				__asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
			}
			sh.last = last;
		}
		__syncthreads();
		if (!sh.last) return;
		finalize_reduce<kIcpThreads>(partials, (int)gridDim.x, sh);
		if (threadIdx.x < 64) finalize_rows(sh.sums, st, *st, (int)threadIdx.x);
	}
}

template <int K, int LAYOUT, bool FUSED, bool CACHE, int LEAVES = 2, bool STRIDED = false, bool ACC = false, bool SLICE = false>
__global__ __launch_bounds__(kIcpThreads, 2048 / kIcpThreads) void icp_pass_kernel(const float4* __restrict__ src, int N,
                                                                  IcpState* __restrict__ st, KdDesc kd, DtDesc dt,
                                                                  float* __restrict__ partials, int* __restrict__ ticket,
                                                                  float4* __restrict__ nn_cache, int* __restrict__ hit_counter, int b0)
{
	icp_pass_body<K, LAYOUT, FUSED, CACHE, LEAVES, STRIDED, ACC, SLICE>(src, N, st, kd, dt, partials, ticket, nn_cache, hit_counter, b0);
}

// ---- trimmed ICP (trim_fraction > 0; jly_icp3d.hpp:236-252): NN for every point, exact selection of
// the `num` smallest squared distances (radix select, ties in point order), sums over the selected ----
template <int K, int LAYOUT>
__global__ __launch_bounds__(kIcpThreads) void icp_nn_kernel(const float4* __restrict__ src, int N,
                                                             const IcpState* __restrict__ st, KdDesc kd, DtDesc dt,
                                                             float* __restrict__ nn_d2, int* __restrict__ nn_slot)
{
	const int lane = threadIdx.x & 63, row = lane >> 4, l = lane & 15;
	const int i = (blockIdx.x * (kIcpThreads / 64) + (threadIdx.x >> 6)) * 4 + row;
	const bool valid = i < N;
	const Box6x4 rootb = load_child_boxes4(kd.boxes[0], l);
	const float4 p = src[valid ? i : N - 1];
	if (st->converged) return;
	const float qx = st->R[0] * p.x + st->R[1] * p.y + st->R[2] * p.z + st->t[0];
	const float qy = st->R[3] * p.x + st->R[4] * p.y + st->R[5] * p.z + st->t[1];
	const float qz = st->R[6] * p.x + st->R[7] * p.y + st->R[8] * p.z + st->t[2];
	const RowNn r = rows_nearest<K, LAYOUT, false, 4>(kd, dt, rootb, l, row, qx, qy, qz, valid);
	if (valid && r.mine) { nn_d2[i] = r.best; nn_slot[i] = r.slot; }
}

// one workgroup: key of the num-th smallest d2 (3-digit radix select), then inclusion flags with the
// ties taken in point order (deterministic)
__global__ __launch_bounds__(1024) void icp_select_stream_kernel(const float* __restrict__ nn_d2, int N, int num,
                                                          const IcpState* __restrict__ st, unsigned char* __restrict__ include)
{
	if (st->converged) return;
	__shared__ unsigned hist[2048];
	__shared__ unsigned sel_prefix, sel_rem, wave_cnt[16], wave_tot[16];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (threadIdx.x == 0) { sel_prefix = 0u; sel_rem = (unsigned)num; }
#pragma unroll 1
	for (int pass = 0; pass < 3; pass++) {
		const int shift = pass == 0 ? 20 : (pass == 1 ? 9 : 0), width = pass == 2 ? 9 : 11, bins = 1 << width;
		for (int i = threadIdx.x; i < 2048; i += 1024) hist[i] = 0u;
		__syncthreads();
		const unsigned prefix = sel_prefix;
		for (int base = 0; base < N; base += 1024) {
			const int i = base + threadIdx.x;
			const unsigned key = i < N ? __float_as_uint(nn_d2[i]) : 0u;
			bool live = i < N && (pass == 0 || (key >> (shift + width)) == prefix);
			const unsigned bin = (key >> shift) & (unsigned)(bins - 1);
			if (live) atomicAdd(&hist[bin], 1u);      // same-address lanes serialise inside LDS (<= 64 cycles per instruction): cheap from registers
		}
		__syncthreads();
		// the bin holding the rem-th smallest candidate: two bins per thread, wavefront scan, 16 wavefront totals
		{
			const unsigned h0 = hist[2 * threadIdx.x], h1 = hist[2 * threadIdx.x + 1];   // bins beyond `bins` are zero
			const unsigned local = h0 + h1;
			unsigned incl = local;
#pragma unroll
			for (int off = 1; off < 64; off <<= 1) {
				const unsigned o = __shfl_up(incl, off, 64);
				if (lane >= off) incl += o;
			}
			if (lane == 63) wave_tot[wave] = incl;
			__syncthreads();
			unsigned before = 0;
			for (int w2 = 0; w2 < wave; w2++) before += wave_tot[w2];
			const unsigned excl = before + incl - local, rem = sel_rem;
			__syncthreads();                                  // every thread has read sel_rem before one rewrites it
			if (excl < rem && rem <= excl + local) {              // exactly one thread
				const bool first = rem <= excl + h0;
				sel_prefix = (prefix << width) | (unsigned)(2 * threadIdx.x + (first ? 0 : 1));
				sel_rem = rem - (first ? excl : excl + h0);
			}
		}
		__syncthreads();
	}
	// inclusion flags; the sel_rem copies of the threshold itself go to the ties that come first in point
	// order: every thread owns a contiguous run of points, counts its ties, one block scan orders them
	const unsigned T = sel_prefix, rem = sel_rem;
	const int per = (N + 1023) / 1024, lo = min((int)threadIdx.x * per, N), hi = min(lo + per, N);
	unsigned mine = 0;
	for (int i = lo; i < hi; i++) mine += __float_as_uint(nn_d2[i]) == T ? 1u : 0u;
	unsigned incl = mine;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const unsigned o = __shfl_up(incl, off, 64);
		if (lane >= off) incl += o;
	}
	if (lane == 63) wave_cnt[wave] = incl;
	__syncthreads();
	unsigned before = incl - mine;
	for (int w2 = 0; w2 < wave; w2++) before += wave_cnt[w2];
	for (int i = lo; i < hi; i++) {
		const unsigned key = __float_as_uint(nn_d2[i]);
		const bool tie = key == T;
		include[i] = (key < T || (tie && before < rem)) ? 1 : 0;
		before += tie ? 1u : 0u;
	}
}

// The same selection for N <= 32 768 with the distances held in registers (32 per thread, one burst of
// loads): a single workgroup streaming them from memory three times is a chain of ~90 dependent loads
// (160 us at bunny size); from registers the three digit passes touch only LDS.
constexpr int kSelPer = 32;
__global__ __launch_bounds__(1024) void icp_select_kernel(const float* __restrict__ nn_d2, int N, int num,
                                                          const IcpState* __restrict__ st, unsigned char* __restrict__ include)
{
	__shared__ unsigned hist[2048];
	__shared__ unsigned sel_prefix, sel_rem, wave_tot[16];
	__shared__ unsigned short tie_cnt[kSelPer][16];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned key[kSelPer];
#pragma unroll
	for (int j = 0; j < kSelPer; j++) {
		const int i = j * 1024 + (int)threadIdx.x;
		key[j] = i < N ? __float_as_uint(nn_d2[i]) : 0xffffffffu;      // padding sorts last (distances are >= 0 and finite)
	}
	if (st->converged) return;
	if (threadIdx.x == 0) { sel_prefix = 0u; sel_rem = (unsigned)num; }
#pragma unroll 1
	for (int pass = 0; pass < 3; pass++) {
		const int shift = pass == 0 ? 20 : (pass == 1 ? 9 : 0), width = pass == 2 ? 9 : 11, bins = 1 << width;
		for (int i = threadIdx.x; i < 2048; i += 1024) hist[i] = 0u;
		__syncthreads();
		const unsigned prefix = sel_prefix;
#pragma unroll
		for (int j = 0; j < kSelPer; j++) {
			const bool live = j * 1024 + (int)threadIdx.x < N && (pass == 0 || (key[j] >> (shift + width)) == prefix);
			const unsigned bin = (key[j] >> shift) & (unsigned)(bins - 1);
			if (live) atomicAdd(&hist[bin], 1u);      // same-address lanes serialise inside LDS (<= 64 cycles per instruction): cheap from registers
		}
		__syncthreads();
		// the bin holding the rem-th smallest candidate: two bins per thread, wavefront scan, 16 wavefront totals
		const unsigned h0 = hist[2 * threadIdx.x], h1 = hist[2 * threadIdx.x + 1];       // bins beyond `bins` are zero
		const unsigned local = h0 + h1;
		unsigned incl = local;
#pragma unroll
		for (int off = 1; off < 64; off <<= 1) {
			const unsigned o = __shfl_up(incl, off, 64);
			if (lane >= off) incl += o;
		}
		if (lane == 63) wave_tot[wave] = incl;
		__syncthreads();
		unsigned before = 0;
		for (int w2 = 0; w2 < wave; w2++) before += wave_tot[w2];
		const unsigned excl = before + incl - local, rem = sel_rem;
		__syncthreads();                                      // every thread has read sel_rem before one rewrites it
		if (excl < rem && rem <= excl + local) {                  // exactly one thread
			const bool first = rem <= excl + h0;
			sel_prefix = (prefix << width) | (unsigned)(2 * threadIdx.x + (first ? 0 : 1));
			sel_rem = rem - (first ? excl : excl + h0);
		}
		__syncthreads();
	}
	// inclusion flags; the sel_rem copies of the threshold itself go to the ties that come first in point order
	// (i = j*1024 + thread): per (j, wavefront) tie counts, one barrier, then every lane ranks its own ties
	const unsigned T = sel_prefix, rem = sel_rem;
#pragma unroll
	for (int j = 0; j < kSelPer; j++) {
		const unsigned long long tb = __ballot(key[j] == T);
		if (lane == 0) tie_cnt[j][wave] = (unsigned short)__popcll(tb);
	}
	__syncthreads();
	// lane j gathers, for iteration j, the ties of the earlier iterations and of the earlier wavefronts
	unsigned wbefore = 0, total = 0;
	if (lane < kSelPer)
		for (int w2 = 0; w2 < 16; w2++) {
			const unsigned c = tie_cnt[lane][w2];
			total += c;
			wbefore += w2 < wave ? c : 0u;
		}
	unsigned incl = total;
#pragma unroll
	for (int off = 1; off < kSelPer; off <<= 1) {
		const unsigned o = __shfl_up(incl, off, 64);
		if (lane >= off) incl += o;
	}
	const unsigned base = incl - total + wbefore;
#pragma unroll
	for (int j = 0; j < kSelPer; j++) {
		const int i = j * 1024 + (int)threadIdx.x;
		const bool tie = key[j] == T;
		const unsigned long long tb = __ballot(tie);
		const unsigned rank = (unsigned)__builtin_amdgcn_readlane((int)base, j) + (unsigned)__popcll(tb & ((1ull << lane) - 1ull));
		if (i < N) include[i] = (key[j] < T || (tie && rank < rem)) ? 1 : 0;
	}
}

__global__ __launch_bounds__(kIcpThreads) void icp_accum_kernel(const float4* __restrict__ src, int N,
                                                                const IcpState* __restrict__ st, KdDesc kd,
                                                                const float* __restrict__ nn_d2, const int* __restrict__ nn_slot,
                                                                const unsigned char* __restrict__ include, float* __restrict__ partials)
{
	__shared__ float red[kIcpThreads / 64][kIcpAcc];
	if (st->converged) return;
	const int i = blockIdx.x * kIcpThreads + threadIdx.x;
	float acc[kIcpAcc];
#pragma unroll
	for (int k = 0; k < kIcpAcc; k++) acc[k] = 0.f;
	if (i < N && include[i]) {
		const float4 p = src[i];
		const float qx = st->R[0] * p.x + st->R[1] * p.y + st->R[2] * p.z + st->t[0];
		const float qy = st->R[3] * p.x + st->R[4] * p.y + st->R[5] * p.z + st->t[1];
		const float qz = st->R[6] * p.x + st->R[7] * p.y + st->R[8] * p.z + st->t[2];
		const float4 m = kd.pts[nn_slot[i]];
		const float ax = qx - st->cq[0], ay = qy - st->cq[1], az = qz - st->cq[2];
		const float bx = m.x - st->cm[0], by = m.y - st->cm[1], bz = m.z - st->cm[2];
		acc[0] = ax; acc[1] = ay; acc[2] = az;
		acc[3] = bx; acc[4] = by; acc[5] = bz;
		acc[6] = ax * bx; acc[7] = ax * by; acc[8] = ax * bz;
		acc[9] = ay * bx; acc[10] = ay * by; acc[11] = ay * bz;
		acc[12] = az * bx; acc[13] = az * by; acc[14] = az * bz;
		acc[15] = nn_d2[i];
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int k = 0; k < kIcpAcc; k++) {
		const float s = wave_sum(acc[k]);
		if (lane == 0) red[wave][k] = s;
	}
	__syncthreads();
	if (threadIdx.x < kIcpAcc) {
		float s = red[0][threadIdx.x];
#pragma unroll
		for (int x = 1; x < kIcpThreads / 64; x++) s += red[x][threadIdx.x];
		partials[(size_t)blockIdx.x * kIcpAcc + threadIdx.x] = s;
	}
}

// Sum the per-block partials in double (fixed order -> deterministic), then -- one lane -- the body of
// the ICP loop after the correspondence pass (jly_icp3d.hpp:253-292): convergence test, means, H,
// SVD, R_ / t_, compose.  The pose lives in device memory, so the host can queue several iterations
// back-to-back without a round trip.  Written for one workgroup of T threads; used by the last workgroup of
// the fused iteration kernel (T = kIcpThreads), by the stand-alone finalize launch (T = kFinThreads; trimmed
// ICP, A/B tests) and by icp_partials_reduce (T = kPreThreads): the same code, but NOT the same summation
// order -- a thread adds the rows r, r + T/4, r + 2 T/4, ..., and T / 64 wavefront totals follow.  A double sum
// of n floats is exact, hence order-free, while the terms' exponents span at most 29 - log2(n) bits, and
// finalize_rows rounds the sums and H to float again, so the fused and the stand-alone form on the same
// rows have given the same states bit for bit in every run compared (tests/test_gpu_icp_forms.py: 17, 65, 257
// and 4 096 rows, whole runs); nothing in the code makes them.  Above 4 096 rows icp_partials_reduce also
// rounds subtotals to float, and the states do differ (seen at 4 097 rows: R by 1.5e-8 after one iteration).

// every thread of the workgroup (T threads); returns with sh.sums[] valid for all threads
template <int T>
__device__ __forceinline__ void finalize_reduce(const float* __restrict__ partials, int nblocks, FinScratch& sh)
{
	// A chain of dependent memory round trips (~1-2 us each: the partials were written by other XCDs), so the loads
	// of a sweep -- eight float4 per thread -- are requested before anything is waited for.  64 row streams x four
	// float4 columns; fixed-order sums (registers, xor-butterfly inside a wavefront, then the wavefront totals in order).
	constexpr int kRows = T / 4;
	const int q = threadIdx.x & 3, r = threadIdx.x >> 2;
	const float4* __restrict__ P = reinterpret_cast<const float4*>(partials);
	double a[4] = {0.0, 0.0, 0.0, 0.0};
	for (int b0 = 0; b0 < nblocks; b0 += kRows * 8) {
		float4 v[8];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const int b = b0 + r + kRows * j;
			v[j] = b < nblocks ? P[(size_t)b * 4 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
		}
#pragma unroll
		for (int j = 0; j < 8; j++) {
			a[0] += (double)v[j].x;
			a[1] += (double)v[j].y;
			a[2] += (double)v[j].z;
			a[3] += (double)v[j].w;
		}
	}
#pragma unroll
	for (int c = 0; c < 4; c++) {
		double x = a[c];
		x += __shfl_xor(x, 4, 64);
		x += __shfl_xor(x, 8, 64);
		x += __shfl_xor(x, 16, 64);
		x += __shfl_xor(x, 32, 64);
		if ((threadIdx.x & 63) < 4) sh.wsum[threadIdx.x >> 6][4 * q + c] = x;
	}
	__syncthreads();
	if (threadIdx.x < kIcpAcc) {
		double t = 0.0;
		for (int i = 0; i < T / 64; i++) t += sh.wsum[i][threadIdx.x];
		sh.sums[threadIdx.x] = t;
	}
	__syncthreads();
}

// ---- the rest of the loop body, three lanes wide ---------------------------------------------------------------
// Lane i (i = 0, 1, 2 of ONE wavefront; the other lanes idle along) owns coordinate i of every vector and row i of every
// 3x3 matrix: the means, H, the one-sided Jacobi SVD (rows of B and V rotate independently; the column inner products
// are three-lane sums taken in the serial order (x0 + x1) + x2), R_ = V diag(1,1,det) U^T, t_, the composed pose.  Same
// arithmetic as a one-lane version, a third of the dependent fp64 chain, and ~40 registers instead of ~150 -- which is
// what lets the correspondence pass carry this code without losing occupancy.
__device__ __forceinline__ double lane_get(double x, int j) { return __shfl(x, j, 64); }
__device__ __forceinline__ float lane_getf(float x, int j) { return __shfl(x, j, 64); }
// lane J of the wavefront, J a constant: two v_readlane_b32 into scalar registers instead of two ds_bpermute_b32 through
// the LDS crossbar (a Jacobi rotation takes three such sums; measured: Kabsch 3.7 -> 2.x us per iteration)
template <int J>
__device__ __forceinline__ double lane_const(double x)
{
	const unsigned long long u = (unsigned long long)__double_as_longlong(x);
	const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, J), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), J);
	return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double sum3(double x) { return (lane_const<0>(x) + lane_const<1>(x)) + lane_const<2>(x); }

// rows of H in (b0, b1, b2) on lanes 0..2 -> row of the Kabsch rotation in r[3]: 3x3 SVD by one-sided Jacobi sweeps in double,
// R = V diag(1,1,det) U^T with the sign on the smallest singular direction (jly_icp3d.hpp:268-285, matrix.cpp:782-808)
__device__ __forceinline__ void kabsch_rows(double b0, double b1, double b2, int row, float r[3])
{
	double v0 = row == 0 ? 1.0 : 0.0, v1 = row == 1 ? 1.0 : 0.0, v2 = row == 2 ? 1.0 : 0.0;
#define GOICP_JACOBI(bp, bq, vp, vq)                                                                        \
	{                                                                                                       \
		const double app = sum3(bp * bp), aqq = sum3(bq * bq), apq = sum3(bp * bq);                         \
		if (!(apq == 0.0 || apq * apq <= 1e-24 * (app * aqq))) {                                            \
			rotated = true;                                                                                 \
			const double da = aqq - app, db = 2 * apq;                                                      \
			const double tn = (da >= 0 ? db : -db) / (fabs(da) + sqrt(da * da + db * db));                  \
			const double cs = rsqrt(1 + tn * tn), sn = cs * tn;                                             \
			const double nbp = cs * bp - sn * bq, nbq = sn * bp + cs * bq;                                  \
			const double nvp = cs * vp - sn * vq, nvq = sn * vp + cs * vq;                                  \
			bp = nbp; bq = nbq; vp = nvp; vq = nvq;                                                         \
		}                                                                                                   \
	}
#pragma unroll 1
	for (int sweep = 0; sweep < 32; sweep++) {
		bool rotated = false;
		GOICP_JACOBI(b0, b1, v0, v1)
		GOICP_JACOBI(b0, b2, v0, v2)
		GOICP_JACOBI(b1, b2, v1, v2)
		if (!rotated) break;
	}
#undef GOICP_JACOBI
	const double n0 = sum3(b0 * b0), n1 = sum3(b1 * b1), n2 = sum3(b2 * b2);
	const double rn0 = n0 > 0 ? rsqrt(n0) : 0.0, rn1 = n1 > 0 ? rsqrt(n1) : 0.0, rn2 = n2 > 0 ? rsqrt(n2) : 0.0;
	const double W0 = n0 * rn0, W1 = n1 * rn1, W2 = n2 * rn2;
	double u0 = b0 * rn0, u1 = b1 * rn1, u2 = b2 * rn2;                       // row `row` of U
	// rank-2 input: the missing left vector is the cross product of the other two (row i needs rows i+1, i+2)
	const int ra = (row + 1) % 3, rb = (row + 2) % 3;
	{
		const double a1 = lane_get(u1, ra), a2 = lane_get(u2, ra), c1 = lane_get(u1, rb), c2 = lane_get(u2, rb);   // U[ra][1], U[ra][2], U[rb][1], U[rb][2]
		const double a0 = lane_get(u0, ra), c0 = lane_get(u0, rb);
		if (!(W0 > 1e-200) && W1 > 1e-200 && W2 > 1e-200) u0 = a1 * c2 - c1 * a2;       // columns a = 1, b = 2
		if (!(W1 > 1e-200) && W2 > 1e-200 && W0 > 1e-200) u1 = a2 * c0 - c2 * a0;       // columns a = 2, b = 0
		if (!(W2 > 1e-200) && W0 > 1e-200 && W1 > 1e-200) u2 = a0 * c1 - c0 * a1;       // columns a = 0, b = 1
	}
	// rank-1 input (every matched target point on one line; exactly so when the line is parallel to an axis): one left vector u, and any
	// orthonormal pair across it completes the basis -- the objective tr(R H) = W_k does not see the choice.  a = e x u, e the axis u has
	// the least of, normalised; b = u x a.  Uniform: the norms and the three components of u are the same in every lane.
	{
		const bool p0 = W0 > 1e-200, p1 = W1 > 1e-200, p2 = W2 > 1e-200;
		const double uk = p0 ? u0 : p1 ? u1 : u2;
		const double x = lane_get(uk, 0), y = lane_get(uk, 1), z = lane_get(uk, 2);
		if ((int)p0 + (int)p1 + (int)p2 == 1) {
			const double fx = fabs(x), fy = fabs(y), fz = fabs(z);
			double ax, ay, az;
			if (fx <= fy && fx <= fz) { ax = 0.0; ay = -z; az = y; }                     // e_x x u
			else if (fy <= fz) { ax = z; ay = 0.0; az = -x; }                            // e_y x u
			else { ax = -y; ay = x; az = 0.0; }                                          // e_z x u
			const double rn = rsqrt(ax * ax + ay * ay + az * az);                        // |e x u|^2 >= 2/3 for a unit u
			ax *= rn; ay *= rn; az *= rn;
			const double bx = y * az - z * ay, by = z * ax - x * az, bz = x * ay - y * ax;
			const double ar = row == 0 ? ax : row == 1 ? ay : az, br = row == 0 ? bx : row == 1 ? by : bz;
			if (p0) { u1 = ar; u2 = br; }
			else if (p1) { u2 = ar; u0 = br; }
			else { u0 = ar; u1 = br; }
		}
	}
	// VUt[row][j] = sum_k V[row][k] U[j][k]
	double vut[3];
#pragma unroll
	for (int j = 0; j < 3; j++) {
		double t = 0;
		t += v0 * lane_get(u0, j);
		t += v1 * lane_get(u1, j);
		t += v2 * lane_get(u2, j);
		vut[j] = t;
	}
	const double m00 = lane_get(vut[0], 0), m01 = lane_get(vut[1], 0), m02 = lane_get(vut[2], 0);
	const double m10 = lane_get(vut[0], 1), m11 = lane_get(vut[1], 1), m12 = lane_get(vut[2], 1);
	const double m20 = lane_get(vut[0], 2), m21 = lane_get(vut[1], 2), m22 = lane_get(vut[2], 2);
	const double det = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
	// the reference sorts singular values in decreasing order (matrix.cpp:782-808): its diag(1,1,det)
	// (jly_icp3d.hpp:268-285) corrects the direction of the smallest one
	int ks = 0;
	double Wk = W0;
	if (W1 < Wk) { ks = 1; Wk = W1; }
	if (W2 < Wk) ks = 2;
#pragma unroll
	for (int j = 0; j < 3; j++) {
		double t = 0;
		t += v0 * (ks == 0 ? det : 1.0) * lane_get(u0, j);
		t += v1 * (ks == 1 ? det : 1.0) * lane_get(u1, j);
		t += v2 * (ks == 2 ? det : 1.0) * lane_get(u2, j);
		r[j] = (float)t;
	}
	// H = 0 has no singular direction at all, and U above is the zero matrix: the rotation of the reference's SVD there is the identity
	// (U = V = I), the step a pure translation.  It is what a single correspondence gives, exactly: the pass centres on the pivot cq =
	// R * centroid + t, which for one point is the moved point itself (the same float expression), so every term of H is an exact 0.
	// Uniform: the norms are wave-wide sums.  (One or two vanishing columns were completed above: the result is a rotation for every finite H.)
	if (n0 == 0.0 && n1 == 0.0 && n2 == 0.0) {                              // exact zeros only: a NaN in H still propagates
#pragma unroll
		for (int j = 0; j < 3; j++) r[j] = row == j ? 1.f : 0.f;
	}
}

// The gated loop's decision after a pass (goicp_set_icp_gate): the inlier count, the truncated cost C = err + (N - n_in) * g2 -- the
// objective sum min(d^2, g2) that gated ICP descends, so the loop does not stop while the inlier set still grows -- and whether to stop:
// too few inliers, or the reference's one-sided test (jly_icp3d.hpp:255) on C.  With n_in = N the term is 0 * g2 = 0: the ungated test, bit for bit.
struct GateStep { int n_in; float cost; bool stop; };
__device__ __forceinline__ GateStep gate_step(const IcpState& rd, float err_new, double count)
{
	GateStep g;
	g.n_in = (int)count;
	g.cost = err_new + (float)((int)rd.n - g.n_in) * rd.g2;
	g.stop = g.n_in < rd.min_inliers || (rd.cost > 0.f && rd.cost - g.cost < rd.err_diff_n);
	return g;
}

// The robust loop's decision after a pass (goicp_set_icp_robust): W = sum w, the robust cost C = sum rho, and whether to stop: W below the metric's
// floor (IcpState::min_inliers), or the reference's one-sided test (jly_icp3d.hpp:255) on C.  While every weight is 1.0f, W is exactly N and C is the
// pass's err from the same integer total: the plain test, bit for bit.
struct RobustStep { double W; float cost; bool stop; };
__device__ __forceinline__ RobustStep robust_step(const IcpState& rd, double W, double C)
{
	RobustStep s;
	s.W = W;
	s.cost = (float)C;
	s.stop = W < (double)rd.min_inliers || (rd.cost > 0.f && rd.cost - s.cost < rd.err_diff_n);
	return s;
}

// called by every lane of ONE wavefront (lanes >= 3 shadow lane 2 and write nothing)
// state: where the new pose is written; rd: where the old one is read -- the stand-alone finalize hands in a copy its threads
// fetched into LDS beside the partial rows (one round trip instead of a chain of four behind the branches below)
// GATE: sums[16] is the pass's inlier count; it takes n's place in the update, and the stop rule is gate_step's
// ROBUST: sums[16] is W, sums[17] is C; W takes n's place (the terms arrive weighted), and the stop rule is robust_step's
template <bool GATE, bool ROBUST>
__device__ __forceinline__ void finalize_rows(const double* __restrict__ sums, IcpState* __restrict__ state, const IcpState& rd, int lane)
{
	const int a = lane < 3 ? lane : 2;
	const bool writer = lane < 3;
	const float err_new = (float)sums[15];
	const int passes = rd.passes + 1;
	GateStep gs{0, 0.f, false};
	if constexpr (GATE) gs = gate_step(rd, err_new, sums[kIcpAcc]);
	RobustStep rs{0.0, 0.f, false};
	if constexpr (ROBUST) rs = robust_step(rd, sums[kIcpAcc], sums[kIcpAcc + 1]);
	if (rd.frozen) {                                                     // timing / scoring only
		if (lane == 0) {
			state->err_new = err_new; state->passes = passes;
			if constexpr (GATE) state->n_in = gs.n_in;
			if constexpr (ROBUST) { state->w_sum = (float)rs.W; state->cost_new = rs.cost; }
		}
		return;
	}
	const float err = rd.err;
	if (GATE ? gs.stop : ROBUST ? rs.stop : (err > 0.f && err - err_new < rd.err_diff_n)) {   // jly_icp3d.hpp:255
		if (lane == 0) {
			state->err_new = err_new; state->passes = passes; state->converged = 1;
			if constexpr (GATE) state->n_in = gs.n_in;
			if constexpr (ROBUST) { state->w_sum = (float)rs.W; state->cost_new = rs.cost; }
		}
		return;
	}
	const double nn = GATE ? (double)gs.n_in : ROBUST ? rs.W : (double)rd.n;
	const float cq = rd.cq[a], cm = rd.cm[a];
	const bool carry = rd.carry_means != 0;
	const double sum_q = sums[a] + nn * (double)cq;
	const double sum_m = sums[3 + a] + nn * (double)cm;
	// jly_icp3d.hpp:244-263: the reference accumulates on top of the previous means and divides by n
	const double carry_d = carry ? (double)rd.mu_d[a] : 0.0;
	const double carry_m = carry ? (double)rd.mu_m[a] : 0.0;
	const float mu_d = (float)((carry_d + sum_q) / nn);
	const float mu_m = (float)((carry_m + sum_m) / nn);
	const double alpha = (double)mu_d - (double)cq, beta = (double)mu_m - (double)cm;
	double h[3];
#pragma unroll
	for (int j = 0; j < 3; j++) {
		const double hj = sums[6 + 3 * a + j] - alpha * sums[3 + j] - sums[a] * lane_get(beta, j) + nn * alpha * lane_get(beta, j);
		h[j] = (double)(float)hj;                                            // the reference holds H in float
	}
	// An H that is nothing but the rounding of its own terms (every correspondence the same target point: the centred target terms are one
	// constant, H is exactly 0 in exact arithmetic and about 2^-24 of a product as summed) has no direction to give: it is taken as the 0 it
	// stands for -- kabsch_rows' identity, a pure translation.  The scale: T = sum |q - cq|^2 + sum |m - cm|^2, from the pass's own sums
	// (sum d^2 = T + n |c|^2 - 2 tr S + 2 c . (sum (q - cq) - sum (m - cm)), c = cq - cm); each of the four terms of an entry of H is at most T / 2
	// (Cauchy-Schwarz) and carries the float rounding of a product and of a row sum of 16, together under 2^-20 T.  A covariance a
	// registration can use is of the order of T.  The robust pass weights the 15 terms and not d^2: no T there, H stays as it is.
	if constexpr (!ROBUST) {
		const double c = (double)cq - (double)cm;
		const double T = sums[15] + 2.0 * sum3(sums[6 + 4 * a]) - nn * sum3(c * c) - 2.0 * sum3(c * (sums[a] - sums[3 + a]));
		const double hm = fmax(fabs(h[0]), fmax(fabs(h[1]), fabs(h[2])));
		if (fmax(lane_const<0>(hm), fmax(lane_const<1>(hm), lane_const<2>(hm))) <= kIcpCovNoise * T) h[0] = h[1] = h[2] = 0.0;
	}
	float Rrow[3];
	kabsch_rows(h[0], h[1], h[2], a, Rrow);
	float oldR[9], oldt[3], sc[3];
#pragma unroll
	for (int k = 0; k < 9; k++) oldR[k] = rd.R[k];
#pragma unroll
	for (int k = 0; k < 3; k++) { oldt[k] = rd.t[k]; sc[k] = rd.src_centroid[k]; }
	float acc = 0.f;
#pragma unroll
	for (int k = 0; k < 3; k++) acc += Rrow[k] * lane_getf(mu_d, k);
	const float t_ = mu_m - acc;                                             // t_ = mu_m - R_ mu_d
	float Rn[3];
#pragma unroll
	for (int j = 0; j < 3; j++) {
		float s2 = 0.f;
#pragma unroll
		for (int k = 0; k < 3; k++) s2 += Rrow[k] * oldR[3 * k + j];
		Rn[j] = s2;                                                          // R <- R_ R
	}
	float s3 = 0.f;
#pragma unroll
	for (int k = 0; k < 3; k++) s3 += Rrow[k] * oldt[k];
	const float tn = s3 + t_;                                                // t <- R_ t + t_
	const float cq_new = Rn[0] * sc[0] + Rn[1] * sc[1] + Rn[2] * sc[2] + tn;
	const int iters = rd.iters + 1;
	if (writer) {
		state->R[3 * a] = Rn[0]; state->R[3 * a + 1] = Rn[1]; state->R[3 * a + 2] = Rn[2];
		state->t[a] = tn; state->cq[a] = cq_new; state->mu_d[a] = mu_d; state->mu_m[a] = mu_m;
	}
	if (lane == 0) {
		state->err = err_new; state->err_new = err_new; state->passes = passes; state->iters = iters;
		if constexpr (GATE) { state->n_in = gs.n_in; state->cost = gs.cost; }
		if constexpr (ROBUST) { state->w_sum = (float)rs.W; state->cost_new = rs.cost; state->cost = rs.cost; }
	}
}

// Large clouds (1 M queries = 62 500 partial rows): a single workgroup reading them all is an 85 us tail on a 1.1 ms pass.
// One more level: workgroup b sums the rows [b * rows_per_block, ...) in double, fixed order, and writes ONE float row; the
// finalize then reads nblocks / rows_per_block rows.
constexpr int kPreThreads = 256, kPreRows = 1024;
__global__ __launch_bounds__(kPreThreads) void icp_partials_reduce(const float* __restrict__ partials, int nblocks, const IcpState* __restrict__ state,
                                                                   float* __restrict__ out)
{
	__shared__ FinScratch sh;
	if (state->converged) return;
	const int b0 = blockIdx.x * kPreRows;
	finalize_reduce<kPreThreads>(partials + (size_t)b0 * kIcpAcc, min(kPreRows, nblocks - b0), sh);
	if (threadIdx.x < kIcpAcc) out[(size_t)blockIdx.x * kIcpAcc + threadIdx.x] = (float)sh.sums[threadIdx.x];
}

__global__ __launch_bounds__(kFinThreads) void icp_finalize_update(const float* __restrict__ partials, int nblocks,
                                                                   IcpState* __restrict__ state)
{
	__shared__ FinScratch sh;
	// the loop state travels to LDS in the same round trip as the flag (one word per thread; finalize_reduce's barriers
	// publish it): finalize_rows then reads it without the chain of dependent global loads its branches would make
	static_assert(sizeof(IcpState) % 4 == 0 && sizeof(IcpState) / 4 <= kFinThreads, "one word per thread");
	if (threadIdx.x < sizeof(IcpState) / 4) reinterpret_cast<unsigned*>(&sh.st)[threadIdx.x] = reinterpret_cast<const unsigned*>(state)[threadIdx.x];
	if (state->converged) return;                 // uniform; the pass kernel left the partials untouched
	finalize_reduce<kFinThreads>(partials, nblocks, sh);
	if (threadIdx.x < 64) finalize_rows(sh.sums, state, sh.st, (int)threadIdx.x);
}

// the finalize of the fixed-point form: 32 replicas x 16 accumulators in, zeroed again on the way out.  ONE wavefront (round 4; it was a
// workgroup of 1 024 threads, one accumulator each): lane t owns accumulator t & 15 of the replicas (t >> 4) + 4 j -- eight loads in flight,
// two shuffles, no cross-wavefront stage -- and a single wavefront finds a free SIMD at once where sixteen had to wait for a whole compute
// unit (tools/overlap_probe.py: beside a bound-evaluation stream the old form waited ~400 us per iteration).  Integer sums: the same totals.
constexpr int kFinAccThreads = 64;
__device__ __forceinline__ void finalize_acc_body(unsigned long long* acc, IcpState* state)
{
	__shared__ double sums[kIcpAcc];
	__shared__ IcpState st;
	static_assert(sizeof(IcpState) / 4 <= kFinAccThreads && (kIcpAccReplicas * kIcpAcc) % kFinAccThreads == 0 && kFinAccThreads / kIcpAcc == 4, "one state word per lane; four replicas per pass of the wavefront");
	const int t = threadIdx.x;
	if (t < (int)(sizeof(IcpState) / 4)) reinterpret_cast<unsigned*>(&st)[t] = reinterpret_cast<const unsigned*>(state)[t];
	if (state->converged) return;                 // uniform; the pass kernel added nothing
	long long v[kIcpAccReplicas * kIcpAcc / kFinAccThreads];
#pragma unroll
	for (int j = 0; j < kIcpAccReplicas * kIcpAcc / kFinAccThreads; j++) v[j] = (long long)acc[kFinAccThreads * j + t];
#pragma unroll
	for (int j = 0; j < kIcpAccReplicas * kIcpAcc / kFinAccThreads; j++) acc[kFinAccThreads * j + t] = 0ull;   // the next pass starts from zero (it cannot start before this kernel has finished)
	long long x = 0;
#pragma unroll
	for (int j = 0; j < kIcpAccReplicas * kIcpAcc / kFinAccThreads; j++) x += v[j];
	x += __shfl_xor(x, 16, 64);
	x += __shfl_xor(x, 32, 64);
	__syncthreads();                              // the state words are in LDS
	if (t < kIcpAcc) sums[t] = (double)x * (double)st.acc_inv;
	__syncthreads();
	finalize_rows(sums, state, st, t);
}
__global__ __launch_bounds__(kFinAccThreads) void icp_finalize_update_acc(unsigned long long* __restrict__ acc, IcpState* __restrict__ state)
{
	finalize_acc_body(acc, state);
}

// ---- the sharded ICP loop (goicp_icp_run_collective): slice pass -> export -> sum over the ranks on the host -> finalize from the sums ----
// the 32 x 16 replicas of the fixed-point pass -> lane t & 15 holds the integer total of accumulator t & 15 (every lane of its column);
// the replicas are zeroed on the way out.  Integer addition wraps, so the order of the adds does not matter.
__device__ __forceinline__ long long acc_take_totals(unsigned long long* __restrict__ acc, int t)
{
	long long v[kIcpAccReplicas * kIcpAcc / kFinAccThreads];
#pragma unroll
	for (int j = 0; j < kIcpAccReplicas * kIcpAcc / kFinAccThreads; j++) v[j] = (long long)acc[kFinAccThreads * j + t];
#pragma unroll
	for (int j = 0; j < kIcpAccReplicas * kIcpAcc / kFinAccThreads; j++) acc[kFinAccThreads * j + t] = 0ull;
	unsigned long long x = 0;
#pragma unroll
	for (int j = 0; j < kIcpAccReplicas * kIcpAcc / kFinAccThreads; j++) x += (unsigned long long)v[j];
	x += (unsigned long long)__shfl_xor((long long)x, 16, 64);
	x += (unsigned long long)__shfl_xor((long long)x, 32, 64);
	return (long long)x;
}
// the loop state to LDS, one word per lane (the caller's barrier publishes it)
__device__ __forceinline__ void icp_state_to_lds(const IcpState* __restrict__ state, IcpState& st, int t)
{
	if (t < (int)(sizeof(IcpState) / 4)) reinterpret_cast<unsigned*>(&st)[t] = reinterpret_cast<const unsigned*>(state)[t];
}

// ONE wavefront: this rank's 16 integer totals and the state's converged flag -> out[0..16] (a small device buffer the host reads back)
__global__ __launch_bounds__(kFinAccThreads) void icp_acc_export_kernel(unsigned long long* __restrict__ acc, const IcpState* __restrict__ state,
                                                                        long long* __restrict__ out)
{
	static_assert((kIcpAccReplicas * kIcpAcc) % kFinAccThreads == 0 && kFinAccThreads / kIcpAcc == 4, "four replicas per pass of the wavefront");
	const int t = threadIdx.x;
	const long long x = acc_take_totals(acc, t);      // a converged state added nothing: the replicas are zero, so are the totals
	if (t < kIcpAcc) out[t] = x;
	if (t == 0) out[kIcpAcc] = state->converged;
	static_assert(sizeof(IcpState) % 4 == 0 && sizeof(IcpState) / 4 <= kFinAccThreads, "one state word per lane");
	if (t < (int)(sizeof(IcpState) / 4)) reinterpret_cast<unsigned*>(out + kIcpAcc + 1)[t] = reinterpret_cast<const unsigned*>(state)[t];
}

// the second half of icp_finalize_update_acc: the 16 totals summed over the ranks -> (double)x * acc_inv -> finalize_rows
__global__ __launch_bounds__(kFinAccThreads) void icp_finalize_from_sums_kernel(const long long* __restrict__ words, IcpState* __restrict__ state)
{
	__shared__ double sums[kIcpAcc];
	__shared__ IcpState st;
	static_assert(sizeof(IcpState) / 4 <= kFinAccThreads, "one state word per lane");
	const int t = threadIdx.x;
	icp_state_to_lds(state, st, t);
	if (state->converged) return;                 // uniform
	const long long x = t < kIcpAcc ? words[t] : 0;
	__syncthreads();                              // the state words are in LDS
	if (t < kIcpAcc) sums[t] = (double)x * (double)st.acc_inv;
	__syncthreads();
	finalize_rows(sums, state, st, t);
}

// test-only entry (goicp_debug_kabsch): the device SVD on a caller-supplied H, one lane
__global__ void kabsch_debug_kernel(const float* __restrict__ H, float* __restrict__ R)
{
	// the production routine: lane i < 3 holds row i of H, gets row i of R (the other lanes shadow lane 2)
	if (blockIdx.x != 0 || threadIdx.x >= 64) return;
	const int a = threadIdx.x < 3 ? (int)threadIdx.x : 2;
	float Rrow[3];
	kabsch_rows((double)H[3 * a], (double)H[3 * a + 1], (double)H[3 * a + 2], a, Rrow);
	if (threadIdx.x < 3) { R[3 * a] = Rrow[0]; R[3 * a + 1] = Rrow[1]; R[3 * a + 2] = Rrow[2]; }
}
hipError_t launch_kabsch_debug(const float* d_H, float* d_R, hipStream_t stream)
{
	hipLaunchKernelGGL(kabsch_debug_kernel, dim3(1), dim3(64), 0, stream, d_H, d_R);
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Gather-ceiling probe (bench.py roofline): the bounds kernel is bound by the vector-memory address /
// L1 path, not by HBM, so its ceiling is measured, in the same run, by a kernel that does nothing
// but issue independent 4-byte loads into the resident distance transform:
//   MODE 0  fully coalesced: the 64 lanes of a wave-instruction read 64 consecutive floats (2 lines)
//   MODE 1  fully divergent: the 64 lanes read 64 different 128-byte lines
// Every workgroup draws its addresses from its own window of `window` floats (a power of two), so the
// footprint per CU -- L1-resident, L2-resident, or the whole grid -- is the caller's choice.  Eight loads
// in flight per lane per iteration, a wave-uniform LCG picks the bases (scalar ALU only).
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void probe_gather_kernel(const float* __restrict__ grid, unsigned n_floats, unsigned window, int iters,
                                                           float* __restrict__ sink)
{
	const unsigned lane = threadIdx.x & 63u;
	const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
	const unsigned span = n_floats - window;
	const unsigned wbase = span ? (unsigned)(((unsigned long long)blockIdx.x * 2654435761ull) % span) & ~63u : 0u;
	const float* __restrict__ w = grid + wbase;
	const unsigned mask = window - 1u;
	unsigned h = __builtin_amdgcn_readfirstlane(wave * 2654435761u + 12345u);
	float acc = 0.f;
	// MODE 0: 64 consecutive floats; MODE 1: 64 lines; MODE k >= 2: k distinct 128-byte lines per instruction, the lanes in
	// k runs of 64/k consecutive floats (lines 8 apart so that neighbouring runs never share a line)
	const unsigned mine = MODE == 0 ? lane : (MODE == 1 ? lane * 32u : (lane / (64u / MODE)) * 256u + (lane % (64u / MODE)));
	for (int it = 0; it < iters; it++) {
		float v[8];
#pragma unroll
		for (int u = 0; u < 8; u++) {
			h = h * 1664525u + 1013904223u;
			const unsigned base = MODE == 1 ? ((h >> 7) & mask) : ((h >> 7) & mask & ~31u);
			v[u] = w[(base + mine) & mask];
		}
#pragma unroll
		for (int u = 0; u < 8; u++) acc += v[u];
	}
	if (acc == 1.2345e-30f) sink[0] = acc;      // never true for a distance field; keeps the loads alive
}

// MODE 2 of the probe: what an LDS-staged DT tile would deliver -- a 64 KiB tile of the grid copied into LDS once, then
// the same independent 4-byte lookups at random tile addresses served by ds_read_b32 (bank conflicts included).
__global__ __launch_bounds__(256) void probe_lds_kernel(const float* __restrict__ grid, unsigned n_floats, int iters, float* __restrict__ sink)
{
	__shared__ float tile[16384];
	const unsigned base = (unsigned)(((unsigned long long)blockIdx.x * 2654435761ull) % (n_floats - 16384u)) & ~63u;
	for (int i = threadIdx.x; i < 16384; i += 256) tile[i] = grid[base + i];
	__syncthreads();
	unsigned h = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u;        // per-lane addresses: a gather
	float acc = 0.f;
	for (int it = 0; it < iters; it++) {
		float v[8];
#pragma unroll
		for (int u = 0; u < 8; u++) {
			h = h * 1664525u + 1013904223u;
			v[u] = tile[(h >> 9) & 16383u];
		}
#pragma unroll
		for (int u = 0; u < 8; u++) acc += v[u];
	}
	if (acc == 1.2345e-30f) sink[0] = acc;
}

hipError_t launch_probe_gather(const DtDesc& dt, int mode, unsigned window, int blocks, int iters, float* sink, hipStream_t stream)
{
	if (mode == 2) {
		const unsigned n = dt.layout ? (unsigned)dt.VB * dt.VB * dt.VB * 64u : (unsigned)dt.V * dt.V * dt.V;
		if (n <= 16384u || dt.layout == 2) return hipErrorInvalidValue;
		hipLaunchKernelGGL(probe_lds_kernel, dim3(blocks), dim3(256), 0, stream, dt.grid, n, iters, sink);
		return hipGetLastError();
	}
	const unsigned n = dt.layout ? (unsigned)dt.VB * dt.VB * dt.VB * 64u : (unsigned)dt.V * dt.V * dt.V;
	if (window < 4096u || (window & (window - 1u)) || window > n) return hipErrorInvalidValue;
	switch (mode) {
	case 0: hipLaunchKernelGGL(probe_gather_kernel<0>, dim3(blocks), dim3(256), 0, stream, dt.grid, n, window, iters, sink); break;
	case 1: hipLaunchKernelGGL(probe_gather_kernel<1>, dim3(blocks), dim3(256), 0, stream, dt.grid, n, window, iters, sink); break;
	case 4: hipLaunchKernelGGL(probe_gather_kernel<4>, dim3(blocks), dim3(256), 0, stream, dt.grid, n, window, iters, sink); break;
	case 8: hipLaunchKernelGGL(probe_gather_kernel<8>, dim3(blocks), dim3(256), 0, stream, dt.grid, n, window, iters, sink); break;
	case 16: hipLaunchKernelGGL(probe_gather_kernel<16>, dim3(blocks), dim3(256), 0, stream, dt.grid, n, window, iters, sink); break;
	case 32: hipLaunchKernelGGL(probe_gather_kernel<32>, dim3(blocks), dim3(256), 0, stream, dt.grid, n, window, iters, sink); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

// A run-time value as a template argument: f(std::integral_constant<int, V>) for the first listed V equal to v, for the last one otherwise.
//   with_k(kd.K, [&](auto K) { launch_x<K()>(...); });
template <int V0, int... Vs, class F>
static void with_value(int v, F&& f)
{
	if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
	else if (v == V0) f(std::integral_constant<int, V0>{});
	else with_value<Vs...>(v, f);
}
template <class F> static void with_k(int K, F&& f) { with_value<1, 2, 3>(K, f); }        // KdDesc::K, the box levels: 1, 2, else 3
template <class F> static void with_flag(bool b, F&& f) { with_value<1, 0>(b, f); }

size_t icp_partials_floats(int N)     // the pass's rows + the rows of the intermediate level (large clouds)
{
	const size_t nb = (size_t)icp_blocks(N);
	return (nb + (nb + kPreRows - 1) / kPreRows) * kIcpAcc;
}

int icp_blocks(int N)
{
	const int per_block = (kIcpThreads / 64) * 4;      // four queries per wavefront
	return (N + per_block - 1) / per_block;
}

// the fixed-point form (bricked DT, two launches per iteration): `acc` is the accumulator block; strangers per wavefront up to
// kIcpStridedMaxN points, neighbours above.  SLICE: workgroups [b0, b0 + nb) of the world-1 grid only (launch_icp_pass_slice)
template <int K, bool SLICE = false>
static void launch_pass_acc(const float4* src, int N, IcpState* st, const KdDesc& kd, const DtDesc& dt, unsigned long long* acc, float4* nn_cache,
                            int* hits, hipStream_t stream, int b0 = 0, int nb = -1)
{
	const dim3 grid(nb < 0 ? icp_blocks(N) : nb), block(kIcpThreads);
	float* a = reinterpret_cast<float*>(acc);
	const bool strided = N <= kIcpStridedMaxN;
	if (nn_cache) {
		if (strided) hipLaunchKernelGGL((icp_pass_kernel<K, 1, false, true, 2, true, true, SLICE>), grid, block, 0, stream, src, N, st, kd, dt, a, nullptr, nn_cache, hits, b0);
		else hipLaunchKernelGGL((icp_pass_kernel<K, 1, false, true, 2, false, true, SLICE>), grid, block, 0, stream, src, N, st, kd, dt, a, nullptr, nn_cache, hits, b0);
	} else {
		if (strided) hipLaunchKernelGGL((icp_pass_kernel<K, 1, false, false, 4, true, true, SLICE>), grid, block, 0, stream, src, N, st, kd, dt, a, nullptr, nn_cache, hits, b0);
		else hipLaunchKernelGGL((icp_pass_kernel<K, 1, false, false, 4, false, true, SLICE>), grid, block, 0, stream, src, N, st, kd, dt, a, nullptr, nn_cache, hits, b0);
	}
}

template <int K, bool FUSED>
static void launch_pass_k(const float4* src, int N, IcpState* st, const KdDesc& kd, const DtDesc& dt, float* partials, int* ticket, float4* nn_cache,
                          int* hits, hipStream_t stream)
{
	const dim3 grid(icp_blocks(N)), block(kIcpThreads);
	if (nn_cache) {
		if (dt.layout) hipLaunchKernelGGL((icp_pass_kernel<K, 1, FUSED, true>), grid, block, 0, stream, src, N, st, kd, dt, partials, ticket, nn_cache, hits, 0);
		else hipLaunchKernelGGL((icp_pass_kernel<K, 0, FUSED, true>), grid, block, 0, stream, src, N, st, kd, dt, partials, ticket, nn_cache, hits, 0);
	} else {
		// four leaves per scan step (S2 845 -> 926 iterations/s, S1 21.9 k -> 23.0 k, bunny 27.0 k -> 27.1 k)
		if (dt.layout) hipLaunchKernelGGL((icp_pass_kernel<K, 1, FUSED, false, FUSED ? 2 : 4>), grid, block, 0, stream, src, N, st, kd, dt, partials, ticket, nn_cache, hits, 0);
		else hipLaunchKernelGGL((icp_pass_kernel<K, 0, FUSED, false, FUSED ? 2 : 4>), grid, block, 0, stream, src, N, st, kd, dt, partials, ticket, nn_cache, hits, 0);
	}
}

template <int K>
static void launch_nn_store_k(const float4* src, int N, IcpState* st, const KdDesc& kd, const DtDesc& dt, float* d2, int* slot, hipStream_t stream)
{
	const dim3 grid(icp_blocks(N)), block(kIcpThreads);
	if (dt.layout) hipLaunchKernelGGL((icp_nn_kernel<K, 1>), grid, block, 0, stream, src, N, st, kd, dt, d2, slot);
	else hipLaunchKernelGGL((icp_nn_kernel<K, 0>), grid, block, 0, stream, src, N, st, kd, dt, d2, slot);
}

int icp_trim_blocks(int N) { return (N + kIcpThreads - 1) / kIcpThreads; }

hipError_t launch_icp_select(const float* nn_d2, int N, int num, const IcpState* st, unsigned char* include, int kernel, hipStream_t stream)
{
	if (kernel == 0) kernel = N <= 1024 * kSelPer ? 1 : 2;
	if (kernel == 1 && N > 1024 * kSelPer) return hipErrorInvalidValue;          // the register kernel holds kSelPer distances per thread
	if (kernel == 1) hipLaunchKernelGGL(icp_select_kernel, dim3(1), dim3(1024), 0, stream, nn_d2, N, num, st, include);
	else hipLaunchKernelGGL(icp_select_stream_kernel, dim3(1), dim3(1024), 0, stream, nn_d2, N, num, st, include);
	return hipGetLastError();
}

hipError_t launch_icp_iteration_trim(const float4* src, int N, int num, IcpState* st, const KdDesc& kd, const DtDesc& dt,
                                     float* nn_d2, int* nn_slot, unsigned char* include, float* partials, hipStream_t stream)
{
	with_k(kd.K, [&](auto K) { launch_nn_store_k<K()>(src, N, st, kd, dt, nn_d2, nn_slot, stream); });
	launch_icp_select(nn_d2, N, num, st, include, 0, stream);
	const int nb = icp_trim_blocks(N);
	hipLaunchKernelGGL(icp_accum_kernel, dim3(nb), dim3(kIcpThreads), 0, stream, src, N, st, kd, nn_d2, nn_slot, include, partials);
	hipLaunchKernelGGL(icp_finalize_update, dim3(1), dim3(kFinThreads), 0, stream, partials, nb, st);
	return hipGetLastError();
}

hipError_t launch_icp_pass_slice(const float4* src, int N, int b0, int b1, IcpState* st, const KdDesc& kd, const DtDesc& dt, unsigned long long* acc,
                                 float4* nn_cache, int* hits, hipStream_t stream)
{
	if (!dt.layout || !acc || b0 < 0 || b1 > icp_blocks(N) || b0 > b1) return hipErrorInvalidValue;
	if (b1 == b0) return hipSuccess;              // an empty range adds nothing: its totals are zero
	with_k(kd.K, [&](auto K) { launch_pass_acc<K(), true>(src, N, st, kd, dt, acc, nn_cache, hits, stream, b0, b1 - b0); });
	return hipGetLastError();
}

hipError_t launch_icp_acc_export(unsigned long long* acc, const IcpState* st, long long* out, hipStream_t stream)
{
	static_assert(kIcpExportWords * 8 >= (kIcpAcc + 1) * 8 + (int)sizeof(IcpState), "export buffer");
	hipLaunchKernelGGL(icp_acc_export_kernel, dim3(1), dim3(kFinAccThreads), 0, stream, acc, st, out);
	return hipGetLastError();
}

long long icp_slice_queries(int N, int b0, int b1)
{
	const int waves = kIcpThreads / 64, nw = (N + 3) >> 2;
	const bool strided = N <= kIcpStridedMaxN;
	long long q = 0;
	for (long long wv = (long long)b0 * waves; wv < (long long)b1 * waves && wv < nw; wv++)
		for (int row = 0; row < 4; row++) q += (strided ? wv + (long long)row * nw : wv * 4 + row) < N;   // icp_pass_kernel's `valid`
	return q;
}

hipError_t launch_icp_finalize_from_sums(const long long* sums16, IcpState* st, hipStream_t stream)
{
	hipLaunchKernelGGL(icp_finalize_from_sums_kernel, dim3(1), dim3(kFinAccThreads), 0, stream, sums16, st);
	return hipGetLastError();
}

// Three forms of one iteration (guard: tests/test_gpu_icp_forms.py).  ticket != nullptr: one fused launch, float rows summed by its last
// workgroup (finalize_reduce<kIcpThreads>); nullptr on the bricked DT with `acc`: the fixed-point pass + icp_finalize_update_acc (the default);
// nullptr otherwise: the float-row pass + stand-alone finalize (finalize_reduce<kFinThreads>, above 4 * kPreRows workgroups behind
// icp_partials_reduce).  The same per-point arithmetic and the same 16-query float row sums in all three; the rows are then added in an order
// of the form's own (see finalize_reduce), so the states of two forms agree within float rounding, not to the bit by construction.
hipError_t launch_icp_iteration(const float4* src, int N, IcpState* st, const KdDesc& kd, const DtDesc& dt, float* partials,
                                int* ticket, float4* nn_cache, int* hits, hipStream_t stream, unsigned long long* acc)
{
	if (!ticket && acc && dt.layout) {
		// the default form: fixed-point sums, no rows of partial sums
		with_k(kd.K, [&](auto K) { launch_pass_acc<K()>(src, N, st, kd, dt, acc, nn_cache, hits, stream); });
		hipLaunchKernelGGL(icp_finalize_update_acc, dim3(1), dim3(kFinAccThreads), 0, stream, acc, st);
		return hipGetLastError();
	}
	if (ticket) {
		with_k(kd.K, [&](auto K) { launch_pass_k<K(), true>(src, N, st, kd, dt, partials, ticket, nn_cache, hits, stream); });
		return hipGetLastError();
	}
	with_k(kd.K, [&](auto K) { launch_pass_k<K(), false>(src, N, st, kd, dt, partials, nullptr, nn_cache, hits, stream); });
	const int nb = icp_blocks(N);
	if (nb > 4 * kPreRows) {
		// two-level sum: the reduced rows live behind the pass's own rows in the same buffer (icp_partials_floats sizes it)
		float* reduced = partials + (size_t)nb * kIcpAcc;
		const int nb2 = (nb + kPreRows - 1) / kPreRows;
		hipLaunchKernelGGL(icp_partials_reduce, dim3(nb2), dim3(kPreThreads), 0, stream, partials, nb, st, reduced);
		hipLaunchKernelGGL(icp_finalize_update, dim3(1), dim3(kFinThreads), 0, stream, reduced, nb2, st);
	} else {
		hipLaunchKernelGGL(icp_finalize_update, dim3(1), dim3(kFinThreads), 0, stream, partials, nb, st);
	}
	return hipGetLastError();
}

__global__ void transform_kernel(float4* __restrict__ src, int N, Pose pose)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= N) return;
	float4 p = src[i];
	float x = pose.R[0] * p.x + pose.R[1] * p.y + pose.R[2] * p.z + pose.t[0];
	float y = pose.R[3] * p.x + pose.R[4] * p.y + pose.R[5] * p.z + pose.t[1];
	float z = pose.R[6] * p.x + pose.R[7] * p.y + pose.R[8] * p.z + pose.t[2];
	src[i] = make_float4(x, y, z, __fsqrt_rn(x * x + y * y + z * z));
}

hipError_t launch_transform(float4* src, int N, const Pose& pose, hipStream_t stream)
{
	if (N <= 0) return hipSuccess;
	hipLaunchKernelGGL(transform_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, src, N, pose);
	return hipGetLastError();
}

// min over n floats and the first index that attains it (what a search does with the upper bounds of a batch: the incumbent
// is the smallest ub, first child on ties -- bnb_queue_kernel's digest; exposed so that a caller driving goicp_eval_bounds_device
// itself, like bench.py's step, reduces with the library's own code).  One workgroup: 65 536 values are 64 per thread, two sweeps of eight
// quads, and a thread issues all the loads of a sweep before it compares any of them (one wait for the memory per sweep, not one per quad).
// the whole sweeps of Q quads per thread that fit between base and n; a thread's indices rise from quad to quad and sweep to sweep, so `<` keeps the first of equal values
template <int Q>
__device__ __forceinline__ void min_sweeps(const float* __restrict__ v, int n, int& base, float& best, int& bi)
{
	for (; n - base >= Q * 4096; base += Q * 4096) {
		float4 x[Q];
#pragma unroll
		for (int k = 0; k < Q; k++) x[k] = *reinterpret_cast<const float4*>(v + base + k * 4096 + (int)threadIdx.x * 4);
#pragma unroll
		for (int k = 0; k < Q; k++) {
			const int i = base + k * 4096 + (int)threadIdx.x * 4;
			if (x[k].x < best) { best = x[k].x; bi = i; }
			if (x[k].y < best) { best = x[k].y; bi = i + 1; }
			if (x[k].z < best) { best = x[k].z; bi = i + 2; }
			if (x[k].w < best) { best = x[k].w; bi = i + 3; }
		}
	}
}
__global__ __launch_bounds__(1024) void reduce_min_kernel(const float* __restrict__ v, int n, float* __restrict__ out_min, int* __restrict__ out_idx)
{
	__shared__ float sv[16];
	__shared__ int si[16];
	// a thread starts at (+inf, its first index): an all-+inf input then yields index 0, not the sentinel of a thread without values
	float best = __builtin_inff();
	int bi = (int)threadIdx.x * 4 < n ? (int)threadIdx.x * 4 : 0x7fffffff;
	int base = 0;
	min_sweeps<8>(v, n, base, best, bi);
	min_sweeps<2>(v, n, base, best, bi);
	// fewer than 8 192 values are left: at most two quads of a thread, and the ragged end value by value
	for (int i = base + (int)threadIdx.x * 4; i < n; i += 4096) {
		if (i + 3 < n) {
			const float4 x = *reinterpret_cast<const float4*>(v + i);
			if (x.x < best) { best = x.x; bi = i; }
			if (x.y < best) { best = x.y; bi = i + 1; }
			if (x.z < best) { best = x.z; bi = i + 2; }
			if (x.w < best) { best = x.w; bi = i + 3; }
		} else
			for (int k = i; k < n; k++) if (v[k] < best) { best = v[k]; bi = k; }
	}
	for (int off = 32; off; off >>= 1) {
		const float ov = __shfl_xor(best, off);
		const int oi = __shfl_xor(bi, off);
		if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
	}
	if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 16; w++) if (sv[w] < best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
		out_min[0] = best;
		if (out_idx) out_idx[0] = bi;
	}
}

hipError_t launch_reduce_min(const float* v, int n, float* out_min, int* out_idx, hipStream_t stream)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(reduce_min_kernel, dim3(1), dim3(1024), 0, stream, v, n, out_min, out_idx);
	return hipGetLastError();
}

template <int K, int LAYOUT>
__global__ __launch_bounds__(kIcpThreads) void nn_query_kernel(const float* __restrict__ q, int n, KdDesc kd, DtDesc dt,
                                                               int32_t* __restrict__ idx, float* __restrict__ d2)
{
	const int lane = threadIdx.x & 63, row = lane >> 4, l = lane & 15;
	const int i = (blockIdx.x * (kIcpThreads / 64) + (threadIdx.x >> 6)) * 4 + row;   // one 16-lane row per query
	const bool valid = i < n;
	const int iq = valid ? i : n - 1;
	const float qx = q[3 * iq], qy = q[3 * iq + 1], qz = q[3 * iq + 2];
	const RowNn r = rows_nearest<K, LAYOUT, false, 4>(kd, dt, load_child_boxes4(kd.boxes[0], l), l, row, qx, qy, qz, valid);
	if (valid && r.mine) { idx[i] = r.idx; d2[i] = r.best; }
}

template <int K>
static void launch_nn_k(const float* q, int n, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2, hipStream_t stream)
{
	const dim3 grid(icp_blocks(n)), block(kIcpThreads);
	if (dt.layout) hipLaunchKernelGGL((nn_query_kernel<K, 1>), grid, block, 0, stream, q, n, kd, dt, idx, d2);
	else hipLaunchKernelGGL((nn_query_kernel<K, 0>), grid, block, 0, stream, q, n, kd, dt, idx, d2);
}

hipError_t launch_nn_query(const float* q, int n, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2, hipStream_t stream)
{
	if (n <= 0) return hipSuccess;
	with_k(kd.K, [&](auto K) { launch_nn_k<K()>(q, n, kd, dt, idx, d2, stream); });
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Exact k nearest target points (k <= kKnnMax) over the same 64-ary box hierarchy, one 16-lane row per query.
// The row keeps its sorted list in registers: lane l holds positions l (`ka`) and l + 16 (`kb`) as 64-bit keys
// (distance bits << 32 | original index) -- distances are >= 0, so the keys order by (d2, index), the tie rule of the
// 1-NN walk.  The walk is rows_nearest's: start from the nearest-point seed (a real candidate), visit child groups in
// ascending box distance, prune against the k-th best distance, scan one leaf (16 slots, one per lane) per step; the
// candidates of a scan that beat the k-th key are inserted one at a time (wave-uniform loop, row-local shuffles).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src)
{
	const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, 64);
	return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long knn_key(float d2, int idx) { return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)idx; }
// the row's key at position kn - 1, in every lane of the row
__device__ __forceinline__ unsigned long long row_kth(unsigned long long ka, unsigned long long kb, int kn, int row)
{
	const int p = kn - 1;
	return shfl_u64(p >= 16 ? kb : ka, row * 16 + (p & 15));
}
// insert the candidate keys `cand` of the row's lanes (~0: none) into the sorted list (ka, kb); candidates at or above the k-th key
// are dropped.  Called by every lane of the wavefront (the loop count is wave-uniform).
__device__ __forceinline__ void knn_insert(unsigned long long cand, unsigned long long& ka, unsigned long long& kb, int kn, int l, int row)
{
	while (true) {
		const unsigned long long kth = row_kth(ka, kb, kn, row);
		const bool pend = cand < kth;
		const unsigned long long bal = __ballot(pend);
		if (bal == 0ull) break;
		const unsigned rb = (unsigned)(bal >> (16 * row)) & 0xffffu;
		const int src = rb ? __ffs((int)rb) - 1 : 0;
		unsigned long long c = shfl_u64(cand, row * 16 + src);
		if (!rb) c = ~0ull;                        // this row has nothing pending: inserting the sentinel changes nothing
		if (rb && l == src) cand = ~0ull;
		const unsigned long long pa = shfl_u64(ka, row * 16 + (l > 0 ? l - 1 : 0));       // position l - 1
		const unsigned long long qb = shfl_u64(kb, row * 16 + (l > 0 ? l - 1 : 0));
		const unsigned long long a15 = shfl_u64(ka, row * 16 + 15);
		const unsigned long long pb = l > 0 ? qb : a15;                                   // position l + 15
		const unsigned long long na = ka < c ? ka : ((l == 0 || pa < c) ? c : pa);
		const unsigned long long nb = kb < c ? kb : (pb < c ? c : pb);
		ka = na; kb = nb;
	}
}

template <int K, int LAYOUT>
__device__ __forceinline__ void rows_knn(const KdDesc& kd, const DtDesc& dt, const Box6x4& rootb, int l, int row, float qx, float qy, float qz,
                                         bool active, int kn, unsigned long long& ka, unsigned long long& kb)
{
	ka = ~0ull; kb = ~0ull;
	if (!__any(active)) return;
	unsigned key[K][4];
	int node[K];
	node[0] = 0;
	boxes_keys4(rootb, qx, qy, qz, key[0]);
#pragma unroll
	for (int L = 1; L < K; L++) {
		node[L] = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) key[L][j] = 0xffffffffu;
	}
	Box6x4 fb = rootb;
	if constexpr (K > 1) {
		row_take(key[0], l, row, node[1]);
		fb = load_child_boxes4(kd.boxes[1] + (size_t)node[1] * 384, l);
	}
	int seed_slot = -1;                            // the seed point enters the list here; its leaf slot is skipped by the scans
	if (dt.nn_ids) {
		const int V1 = dt.V - 1;
		const int ix = min(max((int)rintf((qx - dt.xmin_f) * dt.scale_f), 0), V1);
		const int iy = min(max((int)rintf((qy - dt.ymin_f) * dt.scale_f), 0), V1);
		const int iz = min(max((int)rintf((qz - dt.zmin_f) * dt.scale_f), 0), V1);
		size_t off;
		if (LAYOUT == 0) off = ((size_t)iz * dt.V + iy) * dt.V + ix;
		else off = brick_index(ix, iy, iz, dt.VB);
		const int slot = dt.nn_ids[off];
		const float4 pt = kd.pts[slot];
		const float d0 = qx - pt.x, d1 = qy - pt.y, d2 = qz - pt.z;
		float e = d0 * d0;                                                 // the leaf scan's accumulation order: the same bits
		e += d1 * d1;
		e += d2 * d2;
		if (active && l == 0 && __float_as_int(pt.w) != INT_MAX) ka = knn_key(e, __float_as_int(pt.w));
		seed_slot = slot;
	}
	int d = 0;
	if constexpr (K > 1) {
		boxes_keys4(fb, qx, qy, qz, key[1]);
		d = 1;
	}
	bool done = !active;
	while (__any(!done)) {
		const unsigned bound = (unsigned)(row_kth(ka, kb, kn, row) >> 32);     // bits of the k-th best distance (+inf bits and above: list not full)
		bool acted = done;
		unsigned long long cand = ~0ull;
#pragma unroll
		for (int L = K - 1; L >= 0; L--) {
			if (!acted && d == L) {
				int c;
				const unsigned m = row_take(key[L], l, row, c);
				// A group with nothing left to take is exhausted whatever the bound: while the list is short the bound is 0xffffffff, which
				// no key lies above, and the all-taken key (no real key: box distances are finite or +inf) would otherwise send the row back
				// into child 3 of the group, for ever if that leaf is empty, inserting its points again if not.  Reached by hierarchies whose
				// bottom groups hold fewer than k points (the device build at M / 64^(K-1) < k); k <= M lets every walk fill its list.
				// rows_nearest needs no such test: its bound is a distance from the first step on, finite or +inf, below the all-taken key
				if (m == 0xffffffffu || (m & ~3u) > bound) {
					if (L == 0) { done = true; acted = true; }
					else d = L - 1;
				} else if (L == K - 1) {
					const int s = (node[L] * 64 + c) * kLeafSlots + l;
					const float4 pt = kd.pts[s];
					const float d0 = qx - pt.x, d1 = qy - pt.y, d2 = qz - pt.z;
					float e = d0 * d0;                                      // L2_Simple_Adaptor accumulation order
					e += d1 * d1;
					e += d2 * d2;
					const int id = __float_as_int(pt.w);
					if (s != seed_slot && id != INT_MAX) cand = knn_key(e, id);
					acted = true;
				} else {
					const int NL = L + 1 < K ? L + 1 : L;
					node[NL] = node[L] * 64 + c;
					const Box6x4 cb = load_child_boxes4(kd.boxes[NL] + (size_t)node[NL] * 384, l);
					boxes_keys4(cb, qx, qy, qz, key[NL]);
					d = NL;
					acted = true;
				}
			}
		}
		knn_insert(cand, ka, kb, kn, l, row);
	}
}

template <int K, int LAYOUT>
__global__ __launch_bounds__(kIcpThreads) void knn_query_kernel(const float* __restrict__ q, int n, int kn, KdDesc kd, DtDesc dt,
                                                                int32_t* __restrict__ idx, float* __restrict__ d2)
{
	const int lane = threadIdx.x & 63, row = lane >> 4, l = lane & 15;
	const int i = (blockIdx.x * (kIcpThreads / 64) + (threadIdx.x >> 6)) * 4 + row;
	const bool valid = i < n;
	const int iq = valid ? i : n - 1;
	const float qx = q[3 * iq], qy = q[3 * iq + 1], qz = q[3 * iq + 2];
	unsigned long long ka, kb;
	rows_knn<K, LAYOUT>(kd, dt, load_child_boxes4(kd.boxes[0], l), l, row, qx, qy, qz, valid, kn, ka, kb);
	if (!valid) return;
	if (l < kn) { idx[(size_t)i * kn + l] = (int)(unsigned)ka; d2[(size_t)i * kn + l] = __uint_as_float((unsigned)(ka >> 32)); }
	if (l + 16 < kn) { idx[(size_t)i * kn + l + 16] = (int)(unsigned)kb; d2[(size_t)i * kn + l + 16] = __uint_as_float((unsigned)(kb >> 32)); }
}

template <int K>
static void launch_knn_k(const float* q, int n, int kn, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2, hipStream_t stream)
{
	const dim3 grid(icp_blocks(n)), block(kIcpThreads);
	if (dt.layout) hipLaunchKernelGGL((knn_query_kernel<K, 1>), grid, block, 0, stream, q, n, kn, kd, dt, idx, d2);
	else hipLaunchKernelGGL((knn_query_kernel<K, 0>), grid, block, 0, stream, q, n, kn, kd, dt, idx, d2);
}

hipError_t launch_knn_query(const float* q, int n, int k, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2, hipStream_t stream)
{
	if (k < 1 || k > kKnnMax || k > kd.M) return hipErrorInvalidValue;
	if (n <= 0) return hipSuccess;
	with_k(kd.K, [&](auto K) { launch_knn_k<K()>(q, n, k, kd, dt, idx, d2, stream); });
	return hipGetLastError();
}

// ---- target normals: one row per leaf slot -------------------------------------------------------------------------------
// fp64 3x3 symmetric eigenproblem by cyclic Jacobi rotations: the rotation formula and the stop test of kabsch_rows' one-sided sweeps
// (there on the columns of B, here on the symmetric matrix itself).  a = {a00, a01, a02, a11, a12, a22}; returns the eigenvector of the
// smallest eigenvalue in v and the largest eigenvalue in lmax.
__device__ __forceinline__ void sym3_smallest(const double a_in[6], double v[3], double& lmax)
{
	double A[3][3] = {{a_in[0], a_in[1], a_in[2]}, {a_in[1], a_in[3], a_in[4]}, {a_in[2], a_in[4], a_in[5]}};
	double E[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};        // columns: eigenvectors
	for (int sweep = 0; sweep < 32; sweep++) {
		bool rotated = false;
		for (int pq = 0; pq < 3; pq++) {
			const int p = pq == 2 ? 1 : 0, qq = pq == 0 ? 1 : 2;
			const double app = A[p][p], aqq = A[qq][qq], apq = A[p][qq];
			if (apq == 0.0 || apq * apq <= 1e-24 * fabs(app * aqq)) continue;
			rotated = true;
			// the rotation that zeroes A[p][q]: tan = sign(da) * db / (|da| + sqrt(da^2 + db^2)), da = aqq - app, db = 2 apq
			const double da = aqq - app, db = 2 * apq;
			const double tn = (da >= 0 ? db : -db) / (fabs(da) + sqrt(da * da + db * db));
			const double cs = rsqrt(1 + tn * tn), sn = cs * tn;
			for (int k = 0; k < 3; k++) {                           // A <- A G (columns p, q)
				const double akp = A[k][p], akq = A[k][qq];
				A[k][p] = cs * akp - sn * akq; A[k][qq] = sn * akp + cs * akq;
			}
			for (int k = 0; k < 3; k++) {                           // A <- G^T A (rows p, q)
				const double apk = A[p][k], aqk = A[qq][k];
				A[p][k] = cs * apk - sn * aqk; A[qq][k] = sn * apk + cs * aqk;
			}
			for (int k = 0; k < 3; k++) {
				const double ekp = E[k][p], ekq = E[k][qq];
				E[k][p] = cs * ekp - sn * ekq; E[k][qq] = sn * ekp + cs * ekq;
			}
		}
		if (!rotated) break;
	}
	int ks = 0;
	if (A[1][1] < A[ks][ks]) ks = 1;
	if (A[2][2] < A[ks][ks]) ks = 2;
	lmax = fmax(A[0][0], fmax(A[1][1], A[2][2]));
	v[0] = E[0][ks]; v[1] = E[1][ks]; v[2] = E[2][ks];
}

// row sum of a double over the 16 lanes of a row (fixed butterfly: the same bits in every lane)
__device__ __forceinline__ double row_sum_f64(double x)
{
	x += __shfl_xor(x, 1, 64);
	x += __shfl_xor(x, 2, 64);
	x += __shfl_xor(x, 4, 64);
	x += __shfl_xor(x, 8, 64);
	return x;
}

template <int K, int LAYOUT>
__global__ __launch_bounds__(kIcpThreads) void normal_build_kernel(const float* __restrict__ target, int nslots, int kn, float cx, float cy, float cz,
                                                                   KdDesc kd, DtDesc dt, float4* __restrict__ normals)
{
	const int lane = threadIdx.x & 63, row = lane >> 4, l = lane & 15;
	const int s = (blockIdx.x * (kIcpThreads / 64) + (threadIdx.x >> 6)) * 4 + row;     // leaf slot of this row
	const float4 p = kd.pts[s < nslots ? s : nslots - 1];
	const bool valid = s < nslots && __float_as_int(p.w) != INT_MAX;
	unsigned long long ka, kb;
	rows_knn<K, LAYOUT>(kd, dt, load_child_boxes4(kd.boxes[0], l), l, row, p.x, p.y, p.z, valid, kn, ka, kb);
	// neighbours at positions l and l + 16 (< kn) of the row: their coordinates in fp64; mean, then the covariance about it
	const bool ua = valid && l < kn, ub = valid && l + 16 < kn;
	const int ia = ua ? (int)(unsigned)ka : 0, ib = ub ? (int)(unsigned)kb : 0;
	double xa[3] = {0, 0, 0}, xb[3] = {0, 0, 0};
	if (ua) { xa[0] = target[3 * (size_t)ia]; xa[1] = target[3 * (size_t)ia + 1]; xa[2] = target[3 * (size_t)ia + 2]; }
	if (ub) { xb[0] = target[3 * (size_t)ib]; xb[1] = target[3 * (size_t)ib + 1]; xb[2] = target[3 * (size_t)ib + 2]; }
	double mu[3];
#pragma unroll
	for (int k = 0; k < 3; k++) mu[k] = row_sum_f64(xa[k] + xb[k]) / (double)kn;
	double cov[6];
	{
		const double a0 = ua ? xa[0] - mu[0] : 0.0, a1 = ua ? xa[1] - mu[1] : 0.0, a2 = ua ? xa[2] - mu[2] : 0.0;
		const double b0 = ub ? xb[0] - mu[0] : 0.0, b1 = ub ? xb[1] - mu[1] : 0.0, b2 = ub ? xb[2] - mu[2] : 0.0;
		cov[0] = row_sum_f64(a0 * a0 + b0 * b0);
		cov[1] = row_sum_f64(a0 * a1 + b0 * b1);
		cov[2] = row_sum_f64(a0 * a2 + b0 * b2);
		cov[3] = row_sum_f64(a1 * a1 + b1 * b1);
		cov[4] = row_sum_f64(a1 * a2 + b1 * b2);
		cov[5] = row_sum_f64(a2 * a2 + b2 * b2);
	}
	if (!valid || l != 0) return;
	double v[3], lmax;
	sym3_smallest(cov, v, lmax);
	float n0 = 0.f, n1 = 0.f, n2 = 0.f;
	if (lmax > 1e-30) {
		const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
		n0 = (float)(v[0] / nv); n1 = (float)(v[1] / nv); n2 = (float)(v[2] / nv);
		// sign: n . (p - centroid) >= 0 on the stored floats; a zero product -> the first nonzero component positive
		const double dx = (double)p.x - (double)cx, dy = (double)p.y - (double)cy, dz = (double)p.z - (double)cz;
		double dot = (double)n0 * dx;
		dot += (double)n1 * dy;
		dot += (double)n2 * dz;
		const float first = n0 != 0.f ? n0 : (n1 != 0.f ? n1 : n2);
		if (dot < 0.0 || (dot == 0.0 && first < 0.f)) { n0 = -n0; n1 = -n1; n2 = -n2; }
	}
	normals[__float_as_int(p.w)] = make_float4(n0, n1, n2, 0.f);      // by original index: the pass gathers by the neighbour's index
}

template <int K>
static void launch_normals_k(const float* target, int nslots, int kn, const float c[3], const KdDesc& kd, const DtDesc& dt, float4* normals, hipStream_t stream)
{
	const dim3 grid(icp_blocks(nslots)), block(kIcpThreads);
	if (dt.layout) hipLaunchKernelGGL((normal_build_kernel<K, 1>), grid, block, 0, stream, target, nslots, kn, c[0], c[1], c[2], kd, dt, normals);
	else hipLaunchKernelGGL((normal_build_kernel<K, 0>), grid, block, 0, stream, target, nslots, kn, c[0], c[1], c[2], kd, dt, normals);
}

hipError_t launch_normal_build(const float* target_xyz, int nslots, int k, const float centroid[3], const KdDesc& kd, const DtDesc& dt, float4* normals,
                               hipStream_t stream)
{
	if (k < 1 || k > kKnnMax || k > kd.M || nslots <= 0) return hipErrorInvalidValue;
	with_k(kd.K, [&](auto K) { launch_normals_k<K()>(target_xyz, nslots, k, centroid, kd, dt, normals, stream); });
	return hipGetLastError();
}

// ---- point-to-plane ICP iteration ------------------------------------------------------------------------------------------
// The pass: icp_pass_kernel's query assignment and walk (rows_nearest, four leaves per step, no neighbour cache), so the neighbour and
// its distance are the same bits; the owner lane of a row then forms the row's 28 terms of the Gauss-Newton system linearised about
// the pivot cq (the current transformed source centroid): a = q - cq, r = (q - m) . n, J = (a x n, n) -> the upper triangle of J J^T
// (21), J r (6), d^2.  Float row sums in fixed order per workgroup, then 64-bit fixed-point adds into kIcpAccReplicas x kIcpPlaneStride
// accumulators: integer addition is associative, so the totals do not depend on the arrival order, at any N.
// GATE (goicp_set_icp_gate): the owner zeroes its terms when d^2 > IcpState::g2 and otherwise adds 1 to word 28, the inlier count -- an exact
// float sum of at most 16 ones per workgroup, added unscaled as a plain integer; `capped`: the walk prunes at g2 (rows_nearest<CAP>)
// ROBUST (goicp_set_icp_robust; the plain walk): the 27 terms of J J^T and J r are multiplied by robust_terms' weight of |r| (d^2 stays unweighted),
// each term times its row's weight in the column sums;
// w goes to word 28 (scaled by kIcpRobustWScale), rho -- of the distance d, the quantity the plain plane loop's stop test reads -- to word 29
// SYM (goicp_set_icp_symmetric; include/goicp_mi355.h "symmetric point-to-plane"): the owner also loads the source normal of its query
// (src_normals, parallel to src), rotates it by R, turns it to the target normal's side, and takes n = (s + nm) / 2 and the midpoint
// c = a - e / 2 in the place of nm and a: r = e . n, J = (c x n, n).  |n| <= 1 and c lies between a and m - cq, so the 28 terms keep the plane
// pass's bound; everything after J and r is the plane pass's text
// -> (n, h): h = 0.5f, or 0 where the source normal is exactly zero -- the correspondence is then plain point-to-plane, n = nm and c = a - h e = a
__device__ __forceinline__ float4 symmetric_normal(const float* R, const float4& ns, const float4& nm)
{
	float sx = R[0] * ns.x + R[1] * ns.y + R[2] * ns.z;          // q's row expression without t
	float sy = R[3] * ns.x + R[4] * ns.y + R[5] * ns.z;
	float sz = R[6] * ns.x + R[7] * ns.y + R[8] * ns.z;
	float dot = sx * nm.x;
	dot += sy * nm.y;
	dot += sz * nm.z;
	if (dot < 0.f) { sx = -sx; sy = -sy; sz = -sz; }                  // the same side as the target's normal
	const bool s0 = sx == 0.f && sy == 0.f && sz == 0.f, m0 = nm.x == 0.f && nm.y == 0.f && nm.z == 0.f;
	if (s0) return make_float4(nm.x, nm.y, nm.z, 0.f);                // no source normal: plain point-to-plane (both zero: n = 0)
	if (m0) return make_float4(sx, sy, sz, 0.5f);
	return make_float4(0.5f * (sx + nm.x), 0.5f * (sy + nm.y), 0.5f * (sz + nm.z), 0.5f);
}

// GENERALIZED (goicp_set_icp_generalized; include/goicp_mi355.h "generalized (plane-to-plane) ICP"): the correspondence's 3 x 3 weight
// W = 2 eps Sigma^-1, Sigma = 2 I - (1 - eps) (u u^T + s s^T) with u the target normal and s = R ns, from six cofactors and one determinant, in
// float, operation by operation in the header's order; then the 27 words of the system linearised about the pivot, e' = e + omega x a + tau:
// H_ww = [a]x W [a]x^T (6), H_wt = [a]x W (9), H_tt = W (6) in the upper-triangle order of the plane pass's J J^T, b = (a x g, g), g = W e.
// The words go to the row's LDS line as they are formed: W (6 values) and one row of [a]x W (3) are all that stays live.  W's eigenvalues
// lie in [eps, 1], so every word keeps the plane pass's bound (|n| <= 1 there).  -> e . g, the correspondence's weighted squared residual
__device__ __forceinline__ float generalized_terms(float* dst, const float* R, const float4& ns, const float4& u, float eps, float ax, float ay, float az,
                                                   float ex, float ey, float ez)
{
	const float sx = R[0] * ns.x + R[1] * ns.y + R[2] * ns.z;        // symmetric_normal's row expression
	const float sy = R[3] * ns.x + R[4] * ns.y + R[5] * ns.z;
	const float sz = R[6] * ns.x + R[7] * ns.y + R[8] * ns.z;
	const float k = 1.f - eps, h = 2.f * eps;
	// Sigma: a product of a normal with itself does not see the normal's sign; a zero normal subtracts nothing
	const float Sxx = 2.f - k * (u.x * u.x + sx * sx), Syy = 2.f - k * (u.y * u.y + sy * sy), Szz = 2.f - k * (u.z * u.z + sz * sz);
	const float Sxy = -(k * (u.x * u.y + sx * sy)), Sxz = -(k * (u.x * u.z + sx * sz)), Syz = -(k * (u.y * u.z + sy * sz));
	const float C00 = Syy * Szz - Syz * Syz, C01 = Sxz * Syz - Sxy * Szz, C02 = Sxy * Syz - Sxz * Syy;
	const float C11 = Sxx * Szz - Sxz * Sxz, C12 = Sxy * Sxz - Sxx * Syz, C22 = Sxx * Syy - Sxy * Sxy;
	float det = Sxx * C00;
	det += Sxy * C01;
	det += Sxz * C02;
	const float W00 = (h * C00) / det, W01 = (h * C01) / det, W02 = (h * C02) / det;
	const float W11 = (h * C11) / det, W12 = (h * C12) / det, W22 = (h * C22) / det;
	dst[15] = W00; dst[16] = W01; dst[17] = W02; dst[18] = W11; dst[19] = W12; dst[20] = W22;
	float gx = W00 * ex, gy = W01 * ex, gz = W02 * ex;
	gx += W01 * ey; gy += W11 * ey; gz += W12 * ey;
	gx += W02 * ez; gy += W12 * ez; gz += W22 * ez;
	dst[21] = ay * gz - az * gy;
	dst[22] = az * gx - ax * gz;
	dst[23] = ax * gy - ay * gx;
	dst[24] = gx; dst[25] = gy; dst[26] = gz;
	float eg = ex * gx;
	eg += ey * gy;
	eg += ez * gz;
	// [a]x W row by row (row i = the i-th component of a x column j of W), and that row times [a]x^T
	{
		const float m0 = ay * W02 - az * W01, m1 = ay * W12 - az * W11, m2 = ay * W22 - az * W12;
		dst[0] = m2 * ay - m1 * az; dst[1] = m0 * az - m2 * ax; dst[2] = m1 * ax - m0 * ay;
		dst[3] = m0; dst[4] = m1; dst[5] = m2;
	}
	{
		const float m0 = az * W00 - ax * W02, m1 = az * W01 - ax * W12, m2 = az * W02 - ax * W22;
		dst[6] = m0 * az - m2 * ax; dst[7] = m1 * ax - m0 * ay;
		dst[8] = m0; dst[9] = m1; dst[10] = m2;
	}
	{
		const float m0 = ax * W01 - ay * W00, m1 = ax * W11 - ay * W01, m2 = ax * W12 - ay * W02;
		dst[11] = m1 * ax - m0 * ay;
		dst[12] = m0; dst[13] = m1; dst[14] = m2;
	}
	return eg;
}

// FORM: the plane pass's own (kIcpFormPlane), SYM (kIcpFormSymmetric) or GENERALIZED (kIcpFormGeneralized; gicp_eps is read by it alone)
enum : int { kIcpFormPlane = 0, kIcpFormSymmetric = 1, kIcpFormGeneralized = 2 };
template <int K, int LAYOUT, bool STRIDED, bool GATE = false, bool ROBUST = false, int FORM = kIcpFormPlane>
__device__ __forceinline__ void icp_plane_pass_body(const float4* src, int N, const IcpState* st, const KdDesc& kd, const DtDesc& dt, const float4* normals,
                                                    unsigned long long* acc, int capped = 0, const float4* src_normals = nullptr, float gicp_eps = 0.f)
{
	static_assert(!ROBUST || !GATE, "a robust kernel and a gate exclude each other");
	__shared__ float red[kIcpThreads / 16][kIcpPlaneStride];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane >> 4, l = lane & 15;
	const int gb = (int)blockIdx.x;
	const int nw = (N + 3) >> 2, wv = gb * (kIcpThreads / 64) + wave;
	const int i = STRIDED ? wv + row * nw : wv * 4 + row;
	const bool valid = wv < nw && i < N;
	const Box6x4 rootb = load_child_boxes4(kd.boxes[0], l);
	const int ic = valid ? i : N - 1;
	const float4 p = src[ic];
	if (st->converged) return;
	const float qx = st->R[0] * p.x + st->R[1] * p.y + st->R[2] * p.z + st->t[0];
	const float qy = st->R[3] * p.x + st->R[4] * p.y + st->R[5] * p.z + st->t[1];
	const float qz = st->R[6] * p.x + st->R[7] * p.y + st->R[8] * p.z + st->t[2];
	RowNn r;
	if constexpr (GATE) r = rows_nearest<K, LAYOUT, false, 4, true>(kd, dt, rootb, l, row, qx, qy, qz, valid, capped ? st->g2 : INFINITY);
	else r = rows_nearest<K, LAYOUT, false, 4>(kd, dt, rootb, l, row, qx, qy, qz, valid);
	const int wrow = wave * 4 + row;
	bool owner = valid ? r.mine : l == 0;
	bool inlier = valid;
	if constexpr (GATE) {
		// a capped walk that found nothing inside the gate leaves the row without an owning lane: its lane 0 stores the zeros
		const unsigned mine_row = (unsigned)(__ballot(valid && r.mine) >> (16 * row)) & 0xffffu;
		owner = mine_row ? (valid && r.mine) : l == 0;
		inlier = valid && r.mine && r.best <= st->g2;
	}
	if (owner) {
		// the walk's registers are dead here; the terms go to LDS as they are formed (no array of 28 live values)
		float* dst = red[wrow];
		float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, res = 0.f, d2 = 0.f;
		if (inlier) {
			float4 nm = normals[r.idx];                               // one gather per correspondence (by original index: the walk's slot is dead)
			float ax = qx - st->cq[0], ay = qy - st->cq[1], az = qz - st->cq[2];
			const float ex = qx - r.mx, ey = qy - r.my, ez = qz - r.mz;
			if constexpr (FORM == kIcpFormSymmetric) {
				const float4 ns = src_normals[ic];                    // the query's own normal: one coalesced load (an inlier's ic is its i)
				const float4 n = symmetric_normal(st->R, ns, nm);
				nm.x = n.x; nm.y = n.y; nm.z = n.z;
				ax -= n.w * ex; ay -= n.w * ey; az -= n.w * ez;           // c: the midpoint of the correspondence relative to the pivot
			}
			if constexpr (FORM == kIcpFormGeneralized) {
				// the query's index again (an inlier's is its i), from the lane and wave numbers as the hardware gives them: held across the walk it
				// costs the K = 3 walk, which is at the 64-VGPR bound, a spill
				const int wave2 = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6, row2 = (int)__lane_id() >> 4;
				const int wv2 = gb * (kIcpThreads / 64) + wave2;
				const float4 ns = src_normals[STRIDED ? wv2 + row2 * nw : wv2 * 4 + row2];
				generalized_terms(dst, st->R, ns, nm, gicp_eps, ax, ay, az, ex, ey, ez);   // words 0 .. 26, as they are formed
			} else {
			res = ex * nm.x;
			res += ey * nm.y;
			res += ez * nm.z;
			J[0] = ay * nm.z - az * nm.y;
			J[1] = az * nm.x - ax * nm.z;
			J[2] = ax * nm.y - ay * nm.x;
			J[3] = nm.x; J[4] = nm.y; J[5] = nm.z;
			}
			d2 = r.best;
		}
		if constexpr (FORM == kIcpFormGeneralized) {
			if (!inlier) {
#pragma unroll
				for (int k = 0; k < kIcpPlaneTerms - 1; k++) dst[k] = 0.f;
			}
		} else {
		int k = 0;
#pragma unroll
		for (int a = 0; a < 6; a++)
#pragma unroll
			for (int b = a; b < 6; b++) dst[k++] = J[a] * J[b];
#pragma unroll
		for (int a = 0; a < 6; a++) dst[21 + a] = J[a] * res;
		}
		dst[27] = d2;
		if constexpr (GATE) dst[kIcpPlaneTerms] = inlier ? 1.f : 0.f;
		if constexpr (ROBUST) {
			// the 27 terms go to LDS unweighted and the row's weight beside them: the column sums below multiply (J and the walk's registers are
			// dead by now, so the weight costs no register of the walk's budget)
			RobustTerms rob{0.f, 0.f};                                // a row without a query adds no weight and no cost
			if constexpr (FORM == kIcpFormGeneralized) {
				// the weight of the Euclidean distance, point-to-point's argument: the residual here is a vector
				if (inlier) { const float d = __fsqrt_rn(d2); rob = robust_terms(st->rk, st->rc, d, d, d2); }
			} else {
			if (inlier) rob = robust_terms(st->rk, st->rc, fabsf(res), __fsqrt_rn(d2), d2);
			}
			dst[kIcpPlaneTerms] = rob.w; dst[kIcpPlaneTerms + 1] = rob.rho;
		}
	}
	__syncthreads();
	if (threadIdx.x < kIcpPlaneTerms + (GATE ? 1 : ROBUST ? 2 : 0)) {
		// ROBUST: each of the 27 terms times its row's weight, in float, before the sum (d^2, w and rho as they are)
		const bool weighted = ROBUST && threadIdx.x < kIcpPlaneTerms - 1;
		float sum = weighted ? red[0][threadIdx.x] * red[0][kIcpPlaneTerms] : red[0][threadIdx.x];
#pragma unroll
		for (int x = 1; x < kIcpThreads / 16; x++) sum += weighted ? red[x][threadIdx.x] * red[x][kIcpPlaneTerms] : red[x][threadIdx.x];
		const long long v = GATE && threadIdx.x == kIcpPlaneTerms ? (long long)sum
		                  : __double2ll_rn((double)sum * (ROBUST && threadIdx.x == kIcpPlaneTerms ? kIcpRobustWScale : (double)st->acc_scale));
		unsigned long long* a = acc + (size_t)(gb & (kIcpAccReplicas - 1)) * kIcpPlaneStride + threadIdx.x;
		__hip_atomic_fetch_add(a, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// The pass of every opt-in iteration (launch_icp_iteration_opt): METRIC 0 is the default fixed-point pass (four leaves per step, no neighbour cache:
// every query walks) in its plain, GATE or ROBUST form, METRIC 1 the plane pass; LAYOUT is the DT's (METRIC 1, plain mode; 1 everywhere else).
// BATCH (goicp_icp_run_batch): grid (icp_blocks(N), active poses); blockIdx.y picks a pose slot from the device list `active`, slot s owns states[s]
// and the accumulator block acc + s * kIcpBatchAccWords.  Every workgroup runs the single-pose body on that slot: the same 16 queries, the same float
// row sums, the same acc_scale, the same replica -- and integer addition is associative, so the slot's totals are the single-pose totals bit for bit,
// whatever else the grid holds.  `normals` is read by METRIC 1 and 2 only, `active` by BATCH only, `capped` by the gated mode only.
// METRIC 2 is internal: metric 1 on a handle with goicp_set_icp_symmetric on; `src_normals` (parallel to src) is read by it and METRIC 3.
// METRIC 3 is internal: metric 1 on a handle with goicp_set_icp_generalized on; `gicp_eps` is read by it alone.
template <int K, int LAYOUT, bool STRIDED, int METRIC, int MODE, bool BATCH>
__global__ __launch_bounds__(kIcpThreads, 2048 / kIcpThreads) void icp_opt_pass_kernel(const float4* __restrict__ src, int N,
                                                                      IcpState* __restrict__ states, KdDesc kd, DtDesc dt,
                                                                      const float4* __restrict__ normals, unsigned long long* __restrict__ acc,
                                                                      const int* __restrict__ active, int capped,
                                                                      const float4* __restrict__ src_normals, float gicp_eps)
{
	constexpr bool GATE = MODE == kIcpModeGate, ROBUST = MODE == kIcpModeRobust;
	IcpState* st = states;
	unsigned long long* a = acc;
	if constexpr (BATCH) {
		const int s = active[blockIdx.y];
		st = states + s;
		a = acc + (size_t)s * kIcpBatchAccWords;
	}
	if constexpr (METRIC == 0)
		icp_pass_body<K, 1, false, false, 4, STRIDED, true, false, GATE, ROBUST>(src, N, st, kd, dt, reinterpret_cast<float*>(a), nullptr, nullptr, nullptr, 0, capped);
	else
		icp_plane_pass_body<K, LAYOUT, STRIDED, GATE, ROBUST, METRIC == 3 ? kIcpFormGeneralized : METRIC == 2 ? kIcpFormSymmetric : kIcpFormPlane>(
			src, N, st, kd, dt, normals, a, capped, src_normals, gicp_eps);
}

// fp64 6x6 symmetric eigenproblem by cyclic Jacobi rotations, sym3_smallest's rotation on both sides: S -> diagonal (the eigenvalues), E (the
// identity on entry) -> the eigenvectors in its columns.  A pair whose off-diagonal entry is within `off` is left alone.  Every index is a
// constant once the pair loops are unrolled: both matrices live in registers.
__device__ __forceinline__ void sym6_jacobi(double (&S)[6][6], double (&E)[6][6], double off)
{
#pragma unroll 1
	for (int sweep = 0; sweep < 32; sweep++) {
		bool rotated = false;
#pragma unroll
		for (int p = 0; p < 5; p++) {
#pragma unroll
			for (int q = p + 1; q < 6; q++) {
				const double app = S[p][p], aqq = S[q][q], apq = S[p][q];
				if (!(apq == 0.0 || fabs(apq) <= off)) {
					rotated = true;
					const double da = aqq - app, db = 2 * apq;
					const double tn = (da >= 0 ? db : -db) / (fabs(da) + sqrt(da * da + db * db));
					const double cs = rsqrt(1 + tn * tn), sn = cs * tn;
#pragma unroll
					for (int k = 0; k < 6; k++) {                           // S <- S G (columns p, q)
						const double akp = S[k][p], akq = S[k][q];
						S[k][p] = cs * akp - sn * akq; S[k][q] = sn * akp + cs * akq;
					}
#pragma unroll
					for (int k = 0; k < 6; k++) {                           // S <- G^T S (rows p, q)
						const double apk = S[p][k], aqk = S[q][k];
						S[p][k] = cs * apk - sn * aqk; S[q][k] = sn * apk + cs * aqk;
					}
					S[p][q] = 0.0; S[q][p] = 0.0;
#pragma unroll
					for (int k = 0; k < 6; k++) {
						const double ekp = E[k][p], ekq = E[k][q];
						E[k][p] = cs * ekp - sn * ekq; E[k][q] = sn * ekp + cs * ekq;
					}
				}
			}
		}
		if (!rotated) break;
	}
}

// One wavefront: the replicas -> 28 integer totals (replicas zeroed) -> double; the stop test of finalize_rows; else the damped
// Gauss-Newton step (A + mu I) x = -b by fp64 Cholesky, mu = 1e-12 trace(A); omega = x[0:3], tau = x[3:6]; dR = Rodrigues(omega);
// R <- dR R, t <- dR (t - cq) + cq + tau, cq <- R src_centroid + t.  A system that is rank deficient under kIcpRankTol (a planar target: rank
// 3) takes the minimum-norm step over its retained eigenvalues instead; one with no positive eigenvalue (no usable normal) leaves the pose
// unchanged: the next pass then scores the same error and the loop stops.
// GATE: word 28 is the inlier count (unscaled); the stop rule is gate_step's, the Cholesky system is the one over the inliers as it stands.
// PLANE = false: the same wavefront as the gated POINT-TO-POINT finalize -- the gated pass of either metric adds to kIcpPlaneStride-word
// replicas -- 16 scaled totals and the count in word 16, then finalize_rows<GATE>
// ROBUST: words 28 / 29 (PLANE = false: 16 / 17) are W (scaled by kIcpRobustWScale) and C; the stop rule is robust_step's, the Cholesky system is the
// weighted one as it stands; PLANE = false: finalize_rows<false, true>
template <bool GATE = false, bool PLANE = true, bool ROBUST = false>
__device__ __forceinline__ void icp_plane_finalize_body(unsigned long long* acc, IcpState* state)
{
	static_assert(PLANE || GATE || ROBUST, "the plain point-to-point finalize is finalize_acc_body");
	static_assert(!GATE || !ROBUST, "a robust kernel and a gate exclude each other");
	constexpr int kCountWord = PLANE ? kIcpPlaneTerms : kIcpAcc;
	__shared__ double sums[kIcpPlaneStride];
	__shared__ IcpState st;
	static_assert(sizeof(IcpState) / 4 <= kFinAccThreads && kIcpPlaneStride * 2 == kFinAccThreads, "one state word per lane; two replicas per pass of the wavefront");
	const int t = threadIdx.x;
	icp_state_to_lds(state, st, t);
	if (state->converged) return;                 // uniform; the pass added nothing
	constexpr int kPer = kIcpAccReplicas * kIcpPlaneStride / kFinAccThreads;
	unsigned long long v[kPer];
#pragma unroll
	for (int j = 0; j < kPer; j++) v[j] = acc[kFinAccThreads * j + t];
#pragma unroll
	for (int j = 0; j < kPer; j++) acc[kFinAccThreads * j + t] = 0ull;   // the next pass starts from zero
	unsigned long long x = 0;
#pragma unroll
	for (int j = 0; j < kPer; j++) x += v[j];
	x += (unsigned long long)__shfl_xor((long long)x, 32, 64);
	__syncthreads();                              // the state words are in LDS
	if (t < kIcpPlaneStride)
		sums[t] = GATE && t == kCountWord ? (double)(long long)x
		        : (double)(long long)x * (ROBUST && t == kCountWord ? 1.0 / kIcpRobustWScale : (double)st.acc_inv);
	__syncthreads();
	if constexpr (!PLANE) {
		finalize_rows<GATE, ROBUST>(sums, state, st, t);
		return;
	}
	if (t != 0) return;
	const float err_new = (float)sums[27];
	const int passes = st.passes + 1;
	GateStep gs{0, 0.f, false};
	if constexpr (GATE) gs = gate_step(st, err_new, sums[kIcpPlaneTerms]);
	RobustStep rs{0.0, 0.f, false};
	if constexpr (ROBUST) rs = robust_step(st, sums[kIcpPlaneTerms], sums[kIcpPlaneTerms + 1]);
	if (st.frozen) {
		state->err_new = err_new; state->passes = passes;
		if constexpr (GATE) state->n_in = gs.n_in;
		if constexpr (ROBUST) { state->w_sum = (float)rs.W; state->cost_new = rs.cost; }
		return;
	}
	if (GATE ? gs.stop : ROBUST ? rs.stop : (st.err > 0.f && st.err - err_new < st.err_diff_n)) {   // jly_icp3d.hpp:255, as finalize_rows
		state->err_new = err_new; state->passes = passes; state->converged = 1;
		if constexpr (GATE) state->n_in = gs.n_in;
		if constexpr (ROBUST) { state->w_sum = (float)rs.W; state->cost_new = rs.cost; }
		return;
	}
	// every loop below has constant bounds and is unrolled: the 6x6 system lives in registers (no scratch)
	double A[6][6], b[6];
	{
		int k = 0;
#pragma unroll
		for (int a = 0; a < 6; a++)
#pragma unroll
			for (int c = a; c < 6; c++) { A[a][c] = sums[k]; A[c][a] = sums[k]; k++; }
#pragma unroll
		for (int a = 0; a < 6; a++) b[a] = sums[21 + a];
	}
	double tr = 0.0;
#pragma unroll
	for (int a = 0; a < 6; a++) tr += A[a][a];
	const double mu = 1e-12 * tr;
#pragma unroll
	for (int a = 0; a < 6; a++) A[a][a] += mu;
	// Cholesky A = L L^T in place (lower triangle), then L y = -b, L^T x = y
	bool ok = tr > 0.0;
#pragma unroll
	for (int j = 0; j < 6; j++) {
		double dj = A[j][j];
#pragma unroll
		for (int k = 0; k < j; k++) dj -= A[j][k] * A[j][k];
		ok = ok && dj > 0.0;
		const double ljj = ok ? sqrt(dj) : 1.0;
		A[j][j] = ljj;
#pragma unroll
		for (int i2 = j + 1; i2 < 6; i2++) {
			double s2 = A[i2][j];
#pragma unroll
			for (int k = 0; k < j; k++) s2 -= A[i2][k] * A[j][k];
			A[i2][j] = s2 / ljj;
		}
	}
	double xs[6], y[6];
#pragma unroll
	for (int i2 = 0; i2 < 6; i2++) {
		double s2 = -b[i2];
#pragma unroll
		for (int k = 0; k < i2; k++) s2 -= A[i2][k] * y[k];
		y[i2] = s2 / A[i2][i2];
	}
#pragma unroll
	for (int i2 = 5; i2 >= 0; i2--) {
		double s2 = y[i2];
#pragma unroll
		for (int k = i2 + 1; k < 6; k++) s2 -= A[k][i2] * xs[k];
		xs[i2] = s2 / A[i2][i2];
	}
	// Is the system rank deficient under the rule?  tr(A) tr(A^-1) lies between the condition number and 36 times it (lambda_max <= tr(A) <=
	// 6 lambda_max, the same for A^-1), and tr(A^-1) is the squared Frobenius norm of L^-1: 6 reciprocals and 35 products.  Below the bar the
	// smallest eigenvalue is certainly above the rule and the Cholesky step stands as it is; a failed factorisation or an estimate at the bar
	// (a condition number of at least 1.4e4) sends the system to the eigenvalues, which decide.
	bool trouble = !ok;
	if (ok) {
		double rl[6], tinv = 0.0;
#pragma unroll
		for (int j = 0; j < 6; j++) rl[j] = 1.0 / A[j][j];
#pragma unroll
		for (int c = 0; c < 6; c++) {
			double z[6];                                                 // column c of L^-1
			z[c] = rl[c];
			tinv += z[c] * z[c];
#pragma unroll
			for (int i2 = c + 1; i2 < 6; i2++) {
				double s2 = 0.0;
#pragma unroll
				for (int k = c; k < i2; k++) s2 -= A[i2][k] * z[k];
				z[i2] = s2 * rl[i2];
				tinv += z[i2] * z[i2];
			}
		}
		trouble = !(tr * tinv < 0.5 / kIcpRankTol);
	}
	if (trouble) {
		// the sums again, without the shift; then the eigenvalues: kept are those above kIcpRankTol times the largest.  Full rank: the Cholesky
		// step, untouched.  Else the minimum-norm step x = -sum over the kept (v . b) / lambda v -- no motion along a direction the
		// correspondences do not constrain (a planar target: the turn about its normal and the slide along it)
		double S[6][6], E[6][6];
		{
			int k = 0;
#pragma unroll
			for (int a = 0; a < 6; a++)
#pragma unroll
				for (int c = a; c < 6; c++) { S[a][c] = sums[k]; S[c][a] = sums[k]; k++; }
#pragma unroll
			for (int a = 0; a < 6; a++)
#pragma unroll
				for (int c = 0; c < 6; c++) E[a][c] = a == c ? 1.0 : 0.0;
		}
		int rank = 0;
		double lmax = 0.0;
		if (tr > 0.0) {
			sym6_jacobi(S, E, 1e-16 * tr);
#pragma unroll
			for (int a = 0; a < 6; a++) lmax = fmax(lmax, S[a][a]);
#pragma unroll
			for (int a = 0; a < 6; a++) rank += S[a][a] > kIcpRankTol * lmax ? 1 : 0;
		}
		if (!(ok && rank == 6)) {
			double g[6];
#pragma unroll
			for (int a = 0; a < 6; a++) {
				double s2 = 0.0;
#pragma unroll
				for (int k = 0; k < 6; k++) s2 += E[k][a] * b[k];
				g[a] = lmax > 0.0 && S[a][a] > kIcpRankTol * lmax ? -s2 / S[a][a] : 0.0;
			}
#pragma unroll
			for (int a = 0; a < 6; a++) {
				double s2 = 0.0;
#pragma unroll
				for (int k = 0; k < 6; k++) s2 += E[a][k] * g[k];
				xs[a] = s2;
			}
		}
	}
	// dR = Rodrigues(omega) = I + sin(th)/th W + (1 - cos(th))/th^2 W^2, W = [omega]x
	const double wx = xs[0], wy = xs[1], wz = xs[2];
	const double th = sqrt(wx * wx + wy * wy + wz * wz);
	double dR[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
	if (th > 0.0) {
		const double s1 = sin(th) / th, c1 = (1.0 - cos(th)) / (th * th);
		const double W[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int c = 0; c < 3; c++) {
				double w2 = 0.0;
#pragma unroll
				for (int k = 0; k < 3; k++) w2 += W[a][k] * W[k][c];
				dR[a][c] += s1 * W[a][c] + c1 * w2;
			}
	}
	float Rn[9], tn[3];
#pragma unroll
	for (int a = 0; a < 3; a++) {
#pragma unroll
		for (int c = 0; c < 3; c++) {
			double s2 = 0.0;
#pragma unroll
			for (int k = 0; k < 3; k++) s2 += dR[a][k] * (double)st.R[3 * k + c];
			Rn[3 * a + c] = (float)s2;
		}
		double s3 = 0.0;
#pragma unroll
		for (int k = 0; k < 3; k++) s3 += dR[a][k] * ((double)st.t[k] - (double)st.cq[k]);
		tn[a] = (float)(s3 + (double)st.cq[a] + xs[3 + a]);
	}
#pragma unroll
	for (int a = 0; a < 9; a++) state->R[a] = Rn[a];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		state->t[a] = tn[a];
		state->cq[a] = Rn[3 * a] * st.src_centroid[0] + Rn[3 * a + 1] * st.src_centroid[1] + Rn[3 * a + 2] * st.src_centroid[2] + tn[a];
	}
	state->err = err_new; state->err_new = err_new; state->passes = passes; state->iters = st.iters + 1;
	if constexpr (GATE) { state->n_in = gs.n_in; state->cost = gs.cost; }
	if constexpr (ROBUST) { state->w_sum = (float)rs.W; state->cost_new = rs.cost; state->cost = rs.cost; }
}
// The finalize of every opt-in iteration: one wavefront; BATCH: one per active pose (blockIdx.x indexes the list), on that pose's slot.  Plain
// point-to-point is the default finalize's body, everything else icp_plane_finalize_body<GATE, PLANE, ROBUST>.
template <int METRIC, int MODE, bool BATCH>
__global__ __launch_bounds__(kFinAccThreads) void icp_opt_finalize_kernel(unsigned long long* __restrict__ acc, IcpState* __restrict__ states,
                                                                        const int* __restrict__ active)
{
	IcpState* st = states;
	unsigned long long* a = acc;
	if constexpr (BATCH) {
		const int s = active[blockIdx.x];
		st = states + s;
		a = acc + (size_t)s * kIcpBatchAccWords;
	}
	if constexpr (METRIC == 0 && MODE == kIcpModePlain) finalize_acc_body(a, st);
	else icp_plane_finalize_body<MODE == kIcpModeGate, METRIC != 0, MODE == kIcpModeRobust>(a, st);
}

// ---- the opt-in iterations (point-to-plane, gate, robust kernel; single pose and goicp_icp_run_batch): one pass, then the finalize ----
hipError_t launch_icp_iteration_opt(const IcpOptArgs& a, const KdDesc& kd, const DtDesc& dt, hipStream_t stream)
{
	const bool batch = a.active != nullptr;
	if (!a.states || !a.acc || a.metric < 0 || a.metric > 3 || (a.metric != 0 && !a.normals) || (a.metric >= 2 && !a.src_normals) || a.mode < kIcpModePlain ||
	    a.mode > kIcpModeRobust)
		return hipErrorInvalidValue;
	if (a.metric == 3 && !(a.gicp_eps >= kGicpEpsMin && a.gicp_eps <= 1.f)) return hipErrorInvalidValue;
	if (!dt.layout && (a.metric == 0 || a.mode != kIcpModePlain)) return hipErrorInvalidValue;   // the linear DT: the plain plane pass only
	if (a.n_active < 1 || a.n_active > kIcpBatchMax || (!batch && a.n_active != 1)) return hipErrorInvalidValue;
	if (!batch && a.metric == 0 && a.mode == kIcpModePlain) return hipErrorInvalidValue;         // launch_icp_iteration's
	const dim3 pass_grid(icp_blocks(a.N), a.n_active), fin_grid(a.n_active);
	with_k(kd.K, [&](auto K) {
		with_flag(a.N <= kIcpStridedMaxN, [&](auto S) {       // the default pass's choice: strangers per wavefront for small clouds
			auto go = [&](auto L, auto M, auto MODE, auto B) {
				hipLaunchKernelGGL((icp_opt_pass_kernel<K(), L(), S(), M(), MODE(), B()>), pass_grid, dim3(kIcpThreads), 0, stream, a.src, a.N, a.states, kd, dt,
				                   a.normals, a.acc, a.active, a.capped, a.src_normals, a.gicp_eps);
				hipLaunchKernelGGL((icp_opt_finalize_kernel<M(), MODE(), B()>), fin_grid, dim3(kFinAccThreads), 0, stream, a.acc, a.states, a.active);
			};
			constexpr std::integral_constant<int, 0> c0{};
			constexpr std::integral_constant<int, 1> c1{};
			constexpr std::integral_constant<int, 2> c2{};
			constexpr std::integral_constant<int, 3> c3{};
			// the instantiations: the linear DT with the plain plane pass only; plain point-to-point in a batch only
			if (a.mode != kIcpModePlain)
				with_value<3, 2, 1, 0>(a.metric, [&](auto M) { with_value<kIcpModeGate, kIcpModeRobust>(a.mode, [&](auto MODE) { with_flag(batch, [&](auto B) { go(c1, M, MODE, B); }); }); });
			else if (a.metric == 1)
				with_flag(dt.layout, [&](auto L) { with_flag(batch, [&](auto B) { go(L, c1, c0, B); }); });
			else if (a.metric == 2)
				with_flag(dt.layout, [&](auto L) { with_flag(batch, [&](auto B) { go(L, c2, c0, B); }); });
			else if (a.metric == 3)
				with_flag(dt.layout, [&](auto L) { with_flag(batch, [&](auto B) { go(L, c3, c0, B); }); });
			else
				go(c1, c0, c0, c1);
		});
	});
	return hipGetLastError();
}

// goicp_eval_correspondences: icp_nn_kernel's walk at a pose handed in by value; a neighbour beyond the gate is reported as -1
template <int K, int LAYOUT>
__global__ __launch_bounds__(kIcpThreads) void eval_corr_kernel(const float4* __restrict__ src, int N, Pose pose, float g2, KdDesc kd, DtDesc dt,
                                                                int32_t* __restrict__ idx, float* __restrict__ d2)
{
	const int lane = threadIdx.x & 63, row = lane >> 4, l = lane & 15;
	const int i = (blockIdx.x * (kIcpThreads / 64) + (threadIdx.x >> 6)) * 4 + row;
	const bool valid = i < N;
	const Box6x4 rootb = load_child_boxes4(kd.boxes[0], l);
	const float4 p = src[valid ? i : N - 1];
	// jly_icp3d.hpp:222-224, left-to-right float sums: the pass's own expression, so d2 holds the pass's bits
	const float qx = pose.R[0] * p.x + pose.R[1] * p.y + pose.R[2] * p.z + pose.t[0];
	const float qy = pose.R[3] * p.x + pose.R[4] * p.y + pose.R[5] * p.z + pose.t[1];
	const float qz = pose.R[6] * p.x + pose.R[7] * p.y + pose.R[8] * p.z + pose.t[2];
	const RowNn r = rows_nearest<K, LAYOUT, false, 4>(kd, dt, rootb, l, row, qx, qy, qz, valid);
	if (valid && r.mine) { idx[i] = r.best <= g2 ? r.idx : -1; d2[i] = r.best; }
}

template <int K>
static void launch_eval_corr_k(const float4* src, int N, const Pose& pose, float g2, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2, hipStream_t stream)
{
	const dim3 grid(icp_blocks(N)), block(kIcpThreads);
	if (dt.layout) hipLaunchKernelGGL((eval_corr_kernel<K, 1>), grid, block, 0, stream, src, N, pose, g2, kd, dt, idx, d2);
	else hipLaunchKernelGGL((eval_corr_kernel<K, 0>), grid, block, 0, stream, src, N, pose, g2, kd, dt, idx, d2);
}

hipError_t launch_eval_correspondences(const float4* src, int N, const Pose& pose, float g2, const KdDesc& kd, const DtDesc& dt, int32_t* idx, float* d2,
                                       hipStream_t stream)
{
	if (N <= 0) return hipSuccess;
	if (!idx || !d2) return hipErrorInvalidValue;
	with_k(kd.K, [&](auto K) { launch_eval_corr_k<K()>(src, N, pose, g2, kd, dt, idx, d2, stream); });
	return hipGetLastError();
}

// ---- pose information (goicp_pose_information) ---------------------------------------------------------------------------
// The Gauss-Newton normal matrix and gradient of either metric at a pose handed in by value, about a pivot c: a = q - c, e = q - m.
// The pass is the plane pass's: query assignment, the uncapped walk (rows_nearest, four leaves per step: sse needs every point's d^2, an
// outlier's too, so the gate never caps this walk), the owner lane of a row forms the row's terms and stores them to LDS, float column
// sums over the workgroup's 16 rows in fixed order, 64-bit fixed-point adds into replica (workgroup & 31) of a kIcpPlaneStride block.
// The weight w: 1; [d^2 <= g2] under a gate (g2 = +inf without one); robust_terms' weight under a kernel (rk != 0).
//   METRIC 0 (19 words): W | sum w a (3) | sum w a a^T, upper triangle (6) | sum w a x e (3) | sum w e (3) | sum w d^2 | sum d^2 | n_in;
//            the owner multiplies by w itself: (w a) a^T, w (a x e), w e, w d^2
//   METRIC 1 (31 words): sum w j j^T, upper triangle (21) | sum w j r (6) | sum w r^2 | sum d^2 | W | n_in, j = (a x n, n), r = e . n;
//            the 28 weighted terms go to LDS unweighted and the column sums multiply by the row's w, as the robust plane pass does
// W is scaled by kIcpRobustWScale, n_in (rows with w > 0) is a plain integer, every other word by PoseInfoArgs::scale.
//   METRIC 2 (internal; the symmetric form of metric 1): metric 1's words with n = symmetric_normal and j = (c x n, n), c = a - e / 2,
//            in two phases -- the owner stores the row's raw inputs, pose_info_symmetric_row forms the words behind a barrier
// METRIC 2, second phase: one lane per row turns the row's raw inputs (a, e, nm, d^2, the query's index; the last word: the row has a query)
// into metric 1's 31 words
__device__ __forceinline__ void pose_info_symmetric_row(float* dst, const PoseInfoArgs& pa, const float4* src_normals)
{
	if (dst[kIcpPlaneStride - 1] == 0.f) return;
	float ax = dst[0], ay = dst[1], az = dst[2];
	const float ex = dst[3], ey = dst[4], ez = dst[5], d2 = dst[9];
	const float4 nm = make_float4(dst[6], dst[7], dst[8], 0.f);
	const float4 n = symmetric_normal(pa.R, src_normals[__float_as_int(dst[10])], nm);
	ax -= n.w * ex; ay -= n.w * ey; az -= n.w * ez;           // c: the midpoint of the correspondence relative to the pivot
	float res = ex * n.x;
	res += ey * n.y;
	res += ez * n.z;
	float J[6];
	J[0] = ay * n.z - az * n.y;
	J[1] = az * n.x - ax * n.z;
	J[2] = ax * n.y - ay * n.x;
	J[3] = n.x; J[4] = n.y; J[5] = n.z;
	int k = 0;
#pragma unroll
	for (int a = 0; a < 6; a++)
#pragma unroll
		for (int b = a; b < 6; b++) dst[k++] = J[a] * J[b];
#pragma unroll
	for (int a = 0; a < 6; a++) dst[21 + a] = J[a] * res;
	dst[27] = res * res;
	dst[28] = d2;
	float w = d2 <= pa.g2 ? 1.f : 0.f;
	if (pa.rk) w = robust_terms(pa.rk, pa.rc, fabsf(res), __fsqrt_rn(d2), d2).w;
	dst[29] = w;
	dst[30] = w > 0.f ? 1.f : 0.f;
}
//   METRIC 3 (internal; the generalized form of metric 1): H (21) | b (6) | sum w e^T W e | sum d^2 | W | n_in from generalized_terms, in METRIC 2's
//            two phases; the weight under a kernel is that of the distance d, as in METRIC 0
__device__ __forceinline__ void pose_info_generalized_row(float* dst, const PoseInfoArgs& pa, const float4* src_normals)
{
	if (dst[kIcpPlaneStride - 1] == 0.f) return;
	const float ax = dst[0], ay = dst[1], az = dst[2];
	const float ex = dst[3], ey = dst[4], ez = dst[5], d2 = dst[9];
	const float4 nm = make_float4(dst[6], dst[7], dst[8], 0.f);
	const float4 ns = src_normals[__float_as_int(dst[10])];
	dst[27] = generalized_terms(dst, pa.R, ns, nm, pa.eps, ax, ay, az, ex, ey, ez);   // every input is in a register before the first word is stored
	dst[28] = d2;
	float w = d2 <= pa.g2 ? 1.f : 0.f;
	if (pa.rk) { const float d = __fsqrt_rn(d2); w = robust_terms(pa.rk, pa.rc, d, d, d2).w; }
	dst[29] = w;
	dst[30] = w > 0.f ? 1.f : 0.f;
}
template <int K, int METRIC>
__device__ __forceinline__ void pose_info_body(const float4* src, int N, const PoseInfoArgs& pa, int strided, const KdDesc& kd, const DtDesc& dt,
                                               const float4* normals, unsigned long long* acc, const float4* src_normals = nullptr)
{
	constexpr int kWords = kPoseInfoWords[METRIC];
	constexpr int kWordW = METRIC ? 29 : 0, kWordN = METRIC ? 30 : 18;
	static_assert(kWords <= kIcpPlaneStride, "the words of a replica");
	__shared__ float red[kIcpThreads / 16][kIcpPlaneStride];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane >> 4, l = lane & 15;
	const int gb = (int)blockIdx.x;
	const int nw = (N + 3) >> 2, wv = gb * (kIcpThreads / 64) + wave;
	const int i = strided ? wv + row * nw : wv * 4 + row;
	const bool valid = wv < nw && i < N;
	const Box6x4 rootb = load_child_boxes4(kd.boxes[0], l);
	const float4 p = src[valid ? i : N - 1];
	// jly_icp3d.hpp:222-224, left-to-right float sums: the pass's own expression
	const float qx = pa.R[0] * p.x + pa.R[1] * p.y + pa.R[2] * p.z + pa.t[0];
	const float qy = pa.R[3] * p.x + pa.R[4] * p.y + pa.R[5] * p.z + pa.t[1];
	const float qz = pa.R[6] * p.x + pa.R[7] * p.y + pa.R[8] * p.z + pa.t[2];
	const RowNn r = rows_nearest<K, 1, false, 4>(kd, dt, rootb, l, row, qx, qy, qz, valid);
	const int wrow = wave * 4 + row;
	if (valid ? r.mine : l == 0) {
		float* dst = red[wrow];
		if (!valid) {
#pragma unroll
			for (int k = 0; k < kWords; k++) dst[k] = 0.f;       // a row without a query: no terms, no weight, no count
			if constexpr (METRIC >= 2) dst[kIcpPlaneStride - 1] = 0.f;
		} else {
			const float d2 = r.best;
			const float ax = qx - pa.c[0], ay = qy - pa.c[1], az = qz - pa.c[2];
			const float ex = qx - r.mx, ey = qy - r.my, ez = qz - r.mz;
			if constexpr (METRIC == 0) {
				float w = d2 <= pa.g2 ? 1.f : 0.f;
				if (pa.rk) { const float d = __fsqrt_rn(d2); w = robust_terms(pa.rk, pa.rc, d, d, d2).w; }
				const float wax = w * ax, way = w * ay, waz = w * az;
				dst[0] = w;
				dst[1] = wax; dst[2] = way; dst[3] = waz;
				dst[4] = wax * ax; dst[5] = wax * ay; dst[6] = wax * az;
				dst[7] = way * ay; dst[8] = way * az; dst[9] = waz * az;
				dst[10] = w * (ay * ez - az * ey);
				dst[11] = w * (az * ex - ax * ez);
				dst[12] = w * (ax * ey - ay * ex);
				dst[13] = w * ex; dst[14] = w * ey; dst[15] = w * ez;
				dst[16] = w * d2;
				dst[17] = d2;
				dst[kWordN] = w > 0.f ? 1.f : 0.f;
			} else {
				if constexpr (METRIC >= 2) {
					// the row's raw inputs go to LDS; sixteen lanes form the symmetric (METRIC 3: the generalized) terms from them after the barrier below, so the walk keeps
					// metric 1's registers (its K = 3 form is at the 64-VGPR bound).  The query's index again (a valid row's i is below N), from
					// the lane and wave numbers as the hardware gives them
					const float4 nm = normals[r.idx];
					const int wave2 = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6, row2 = (int)__lane_id() >> 4;
					const int wv2 = gb * (kIcpThreads / 64) + wave2;
					dst[0] = ax; dst[1] = ay; dst[2] = az; dst[3] = ex; dst[4] = ey; dst[5] = ez;
					dst[6] = nm.x; dst[7] = nm.y; dst[8] = nm.z; dst[9] = d2;
					dst[10] = __int_as_float(strided ? wv2 + row2 * nw : wv2 * 4 + row2);
					static_assert(kWords < kIcpPlaneStride, "the row's spare word");
					dst[kIcpPlaneStride - 1] = 1.f;
				} else {
				const float4 nm = normals[r.idx];                     // by original index, as the plane pass gathers it
				float res = ex * nm.x;
				res += ey * nm.y;
				res += ez * nm.z;
				float J[6];
				J[0] = ay * nm.z - az * nm.y;
				J[1] = az * nm.x - ax * nm.z;
				J[2] = ax * nm.y - ay * nm.x;
				J[3] = nm.x; J[4] = nm.y; J[5] = nm.z;
				int k = 0;
#pragma unroll
				for (int a = 0; a < 6; a++)
#pragma unroll
					for (int b = a; b < 6; b++) dst[k++] = J[a] * J[b];
#pragma unroll
				for (int a = 0; a < 6; a++) dst[21 + a] = J[a] * res;
				dst[27] = res * res;
				dst[28] = d2;
				float w = d2 <= pa.g2 ? 1.f : 0.f;
				if (pa.rk) w = robust_terms(pa.rk, pa.rc, fabsf(res), __fsqrt_rn(d2), d2).w;
				dst[kWordW] = w;
				dst[kWordN] = w > 0.f ? 1.f : 0.f;
				}
			}
		}
	}
	__syncthreads();
	if constexpr (METRIC == 2) {
		if (threadIdx.x < kIcpThreads / 16) pose_info_symmetric_row(red[threadIdx.x], pa, src_normals);
		__syncthreads();
	}
	if constexpr (METRIC == 3) {
		if (threadIdx.x < kIcpThreads / 16) pose_info_generalized_row(red[threadIdx.x], pa, src_normals);
		__syncthreads();
	}
	if (threadIdx.x < kWords) {
		const bool weighted = METRIC != 0 && threadIdx.x < 28;
		float sum = weighted ? red[0][threadIdx.x] * red[0][kWordW] : red[0][threadIdx.x];
#pragma unroll
		for (int x = 1; x < kIcpThreads / 16; x++) sum += weighted ? red[x][threadIdx.x] * red[x][kWordW] : red[x][threadIdx.x];
		const long long v = threadIdx.x == kWordN ? (long long)sum
		                  : __double2ll_rn((double)sum * (threadIdx.x == kWordW ? kIcpRobustWScale : (double)pa.scale));
		unsigned long long* a = acc + (size_t)(gb & (kIcpAccReplicas - 1)) * kIcpPlaneStride + threadIdx.x;
		__hip_atomic_fetch_add(a, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

template <int K, int METRIC>
__global__ __launch_bounds__(kIcpThreads, 2048 / kIcpThreads) void pose_info_kernel(const float4* __restrict__ src, int N, PoseInfoArgs pa, int strided,
                                                                  KdDesc kd, DtDesc dt, const float4* __restrict__ normals,
                                                                  unsigned long long* __restrict__ acc, const float4* __restrict__ src_normals)
{
	pose_info_body<K, METRIC>(src, N, pa, strided, kd, dt, normals, acc, src_normals);
}

// goicp_pose_information_batch: blockIdx.y is the pose slot -- its argument block args[slot], its accumulator block acc + slot * kIcpBatchAccWords.
// The body, the queries of a workgroup, the replica and the scale are the single call's, so a slot's integer totals are the single call's bit for bit.
template <int K, int METRIC>
__global__ __launch_bounds__(kIcpThreads, 2048 / kIcpThreads) void pose_info_batch_kernel(const float4* __restrict__ src, int N,
                                                                        const PoseInfoArgs* __restrict__ args, int strided, KdDesc kd, DtDesc dt,
                                                                        const float4* __restrict__ normals, unsigned long long* __restrict__ acc,
                                                                        const float4* __restrict__ src_normals)
{
	const int s = (int)blockIdx.y;
	pose_info_body<K, METRIC>(src, N, args[s], strided, kd, dt, normals, acc + (size_t)s * kIcpBatchAccWords, src_normals);
}

template <int K>
static void launch_pose_info_k(const float4* src, int N, const PoseInfoArgs* h_args, const PoseInfoArgs* d_args, int n_poses, int metric, const KdDesc& kd,
                               const DtDesc& dt, const float4* normals, unsigned long long* acc, const float4* src_normals, hipStream_t stream)
{
	const dim3 block(kIcpThreads);
	const int strided = N <= kIcpStridedMaxN ? 1 : 0;        // the ICP passes' choice
	with_value<3, 2, 1, 0>(metric, [&](auto M) {
		if (h_args)
			hipLaunchKernelGGL((pose_info_kernel<K, M()>), dim3(icp_blocks(N)), block, 0, stream, src, N, *h_args, strided, kd, dt, normals, acc, src_normals);
		else
			hipLaunchKernelGGL((pose_info_batch_kernel<K, M()>), dim3(icp_blocks(N), n_poses), block, 0, stream, src, N, d_args, strided, kd, dt, normals, acc,
			                   src_normals);
	});
}

static hipError_t launch_pose_info_any(const float4* src, int N, const PoseInfoArgs* h_args, const PoseInfoArgs* d_args, int n_poses, int metric,
                                       const KdDesc& kd, const DtDesc& dt, const float4* normals, unsigned long long* acc, const float4* src_normals,
                                       hipStream_t stream)
{
	if (N <= 0 || !acc || !dt.layout || metric < 0 || metric > 3 || (metric != 0 && !normals) || (metric >= 2 && !src_normals) || n_poses < 1 ||
	    n_poses > kIcpBatchMax)
		return hipErrorInvalidValue;
	with_k(kd.K, [&](auto K) { launch_pose_info_k<K()>(src, N, h_args, d_args, n_poses, metric, kd, dt, normals, acc, src_normals, stream); });
	return hipGetLastError();
}

hipError_t launch_pose_info(const float4* src, int N, const PoseInfoArgs& args, int metric, const KdDesc& kd, const DtDesc& dt, const float4* normals,
                            unsigned long long* acc, hipStream_t stream, const float4* src_normals)
{
	return launch_pose_info_any(src, N, &args, nullptr, 1, metric, kd, dt, normals, acc, src_normals, stream);
}

hipError_t launch_pose_info_batch(const float4* src, int N, const PoseInfoArgs* d_args, int n_poses, int metric, const KdDesc& kd, const DtDesc& dt,
                                  const float4* normals, unsigned long long* acc, hipStream_t stream, const float4* src_normals)
{
	if (!d_args) return hipErrorInvalidValue;
	return launch_pose_info_any(src, N, nullptr, d_args, n_poses, metric, kd, dt, normals, acc, src_normals, stream);
}

// ---- source normals into the order of the source (goicp_set_icp_symmetric) ---------------------------------------------------------------
// out[i] = (normal of point perm[i], 0): the float4 array parallel to src that the symmetric pass loads by query.  nrm: 3 n floats in the
// caller's point order (launch_estimate_normals' output, or the caller's own normals); perm: launch_source_order's permutation
__global__ __launch_bounds__(256) void source_normals_gather_kernel(const float* __restrict__ nrm, const int32_t* __restrict__ perm, int n,
                                                                    float4* __restrict__ out)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const size_t o = 3 * (size_t)perm[i];
	out[i] = make_float4(nrm[o], nrm[o + 1], nrm[o + 2], 0.f);
}

hipError_t launch_source_normals_gather(const float* d_normals_xyz, const int32_t* d_perm, int n, float4* d_out, hipStream_t stream)
{
	if (n <= 0) return hipSuccess;
	if (!d_normals_xyz || !d_perm || !d_out) return hipErrorInvalidValue;
	hipLaunchKernelGGL(source_normals_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_normals_xyz, d_perm, n, d_out);
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Exact Euclidean distance transform of the seed grid (replaces DT3D::Build's 8-pass propagation,
// jly_3ddt.cpp:710-742; same bbox/expand/cubify/int(x+0.5) seeding, jly_3ddt.cpp:889-965).
// Squared distances are integers, so the three separable min-plus passes are exact.
// ------------------------------------------------------------------------------------------------
constexpr int kEdtInf = 1 << 28;

__global__ void dt_fill_kernel(int32_t* __restrict__ w, size_t n)
{
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	for (; i < n; i += (size_t)gridDim.x * blockDim.x) w[i] = kEdtInf;
}

__global__ void dt_seed_kernel(const float* __restrict__ m, int M, DtDesc dt, int32_t* __restrict__ w)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= M) return;
	// the model floats are widened to double before the index math (jly_goicp.cpp:80-85, jly_3ddt.cpp:954-956)
	int x = (int)(((double)m[3 * i] - dt.xmin) * dt.scale + 0.5);
	int y = (int)(((double)m[3 * i + 1] - dt.ymin) * dt.scale + 0.5);
	int z = (int)(((double)m[3 * i + 2] - dt.zmin) * dt.scale + 0.5);
	const int V = dt.V;
	if (x < 0 || x >= V || y < 0 || y >= V || z < 0 || z >= V) return;   // :958
	w[((size_t)z * V + y) * V + x] = 0;                                    // benign race: every writer stores 0
}

// one block per grid row along `axis`; out[x] = min_i (x-i)^2 + g[i]; the row lives in LDS and
// the inner read is a broadcast.
__global__ __launch_bounds__(256) void dt_pass_kernel(int32_t* __restrict__ w, int V, int axis)
{
	extern __shared__ int32_t row[];
	const int r = blockIdx.x;
	size_t base, stride;
	if (axis == 0) { base = (size_t)r * V; stride = 1; }
	else if (axis == 1) { int z = r / V, x = r - z * V; base = (size_t)z * V * V + x; stride = V; }
	else { base = r; stride = (size_t)V * V; }
	for (int i = threadIdx.x; i < V; i += blockDim.x) row[i] = w[base + i * stride];
	__syncthreads();
	for (int x = threadIdx.x; x < V; x += blockDim.x) {
		int best = kEdtInf;
		for (int i = 0; i < V; i++) {
			int d = x - i;
			int v = d * d + row[i];
			best = v < best ? v : best;
		}
		w[base + x * stride] = best;
	}
}

template <int LAYOUT>
__global__ void dt_finish_kernel(const int32_t* w, DtDesc dt, float* out)
{
	const int V = dt.V;
	size_t n = (size_t)V * V * V;
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	// jly_3ddt.cpp:967-978: the float holding sqrt(v^2+h^2+d^2), divided by the double scale
	float dist = (float)sqrt((double)w[i]);
	float v = (float)((double)dist / dt.scale);
	if (v < 0.f) v = 0.f;
	if (LAYOUT == 0) {
		out[i] = v;
	} else {
		int x = (int)(i % V), y = (int)((i / V) % V), z = (int)(i / ((size_t)V * V));
		out[brick_index(x, y, z, dt.VB)] = v;
	}
}

// ---- nearest-target-point table: the EDT passes again, carrying which seed attains the minimum ----
__global__ void nnseed_fill_kernel(int32_t* __restrict__ w, int32_t* __restrict__ id, size_t n)
{
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	for (; i < n; i += (size_t)gridDim.x * blockDim.x) { w[i] = kEdtInf; id[i] = 0x7fffffff; }
}
__global__ void nnseed_seed_kernel(const float4* __restrict__ pts, int nslots, DtDesc dt, int32_t* __restrict__ w, int32_t* __restrict__ id)
{
	const int s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nslots) return;
	const float4 p = pts[s];
	if (!(p.x < INFINITY)) return;                                            // padding slot
	const int x = (int)(((double)p.x - dt.xmin) * dt.scale + 0.5);          // the seeding rule of the distance transform (dt_seed_kernel)
	const int y = (int)(((double)p.y - dt.ymin) * dt.scale + 0.5);
	const int z = (int)(((double)p.z - dt.zmin) * dt.scale + 0.5);
	const int V = dt.V;
	if (x < 0 || x >= V || y < 0 || y >= V || z < 0 || z >= V) return;
	const size_t v = ((size_t)z * V + y) * V + x;
	w[v] = 0;
	atomicMin(&id[v], s);                                                     // lowest slot: the table is reproducible
}
__global__ __launch_bounds__(256) void nnseed_pass_kernel(int32_t* __restrict__ w, int32_t* __restrict__ id, int V, int axis)
{
	extern __shared__ int32_t row[];                                          // [V] distances, [V] ids
	int32_t* idrow = row + V;
	const int r = blockIdx.x;
	size_t base, stride;
	if (axis == 0) { base = (size_t)r * V; stride = 1; }
	else if (axis == 1) { int z = r / V, x = r - z * V; base = (size_t)z * V * V + x; stride = V; }
	else { base = r; stride = (size_t)V * V; }
	for (int i = threadIdx.x; i < V; i += blockDim.x) { row[i] = w[base + i * stride]; idrow[i] = id[base + i * stride]; }
	__syncthreads();
	for (int x = threadIdx.x; x < V; x += blockDim.x) {
		int best = kEdtInf, bi = x;
		for (int i = 0; i < V; i++) {
			const int d = x - i;
			const int v = d * d + row[i];
			if (v < best) { best = v; bi = i; }
		}
		w[base + x * stride] = best;
		id[base + x * stride] = idrow[bi];
	}
}
template <int LAYOUT>
__global__ void nnseed_finish_kernel(const int32_t* __restrict__ id, DtDesc dt, int32_t* __restrict__ out)
{
	const int V = dt.V;
	const size_t n = (size_t)V * V * V;
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	if (LAYOUT == 0) { out[i] = id[i]; return; }
	const int x = (int)(i % V), y = (int)((i / V) % V), z = (int)(i / ((size_t)V * V));
	out[brick_index(x, y, z, dt.VB)] = id[i];
}
hipError_t launch_nn_seed_build(const float4* pts, int nslots, const DtDesc& dt, int32_t* work_d, int32_t* work_id, int32_t* out, hipStream_t stream)
{
	const int V = dt.V;
	const size_t n = (size_t)V * V * V;
	hipLaunchKernelGGL(nnseed_fill_kernel, dim3(4096), dim3(256), 0, stream, work_d, work_id, n);
	hipLaunchKernelGGL(nnseed_seed_kernel, dim3((nslots + 255) / 256), dim3(256), 0, stream, pts, nslots, dt, work_d, work_id);
	for (int axis = 0; axis < 3; axis++)
		hipLaunchKernelGGL(nnseed_pass_kernel, dim3(V * V), dim3(256), 2 * V * sizeof(int32_t), stream, work_d, work_id, V, axis);
	const dim3 grid((unsigned)((n + 255) / 256));
	if (dt.layout == 0) hipLaunchKernelGGL(nnseed_finish_kernel<0>, grid, dim3(256), 0, stream, work_id, dt, out);
	else hipLaunchKernelGGL(nnseed_finish_kernel<1>, grid, dim3(256), 0, stream, work_id, dt, out);
	return hipGetLastError();
}

// half-precision copy of a bricked grid, rounded toward zero (|half| <= |float|: lower bounds stay valid)
__global__ void dt_to_half_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, size_t n)
{
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	for (; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = __half_as_ushort(__float2half_rz(in[i]));
}
hipError_t launch_dt_to_half(const float* bricked, void* out_half, size_t n, hipStream_t stream)
{
	hipLaunchKernelGGL(dt_to_half_kernel, dim3(4096), dim3(256), 0, stream, bricked, static_cast<unsigned short*>(out_half), n);
	return hipGetLastError();
}

hipError_t launch_dt_build(const float* model_xyz, int M, const DtDesc& dt, int32_t* work, float* out, hipStream_t stream)
{
	const int V = dt.V;
	const size_t n = (size_t)V * V * V;
	hipLaunchKernelGGL(dt_fill_kernel, dim3(4096), dim3(256), 0, stream, work, n);
	hipLaunchKernelGGL(dt_seed_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, model_xyz, M, dt, work);
	for (int axis = 0; axis < 3; axis++)
		hipLaunchKernelGGL(dt_pass_kernel, dim3(V * V), dim3(256), V * sizeof(int32_t), stream, work, V, axis);
	dim3 grid((unsigned)((n + 255) / 256));
	if (dt.layout == 0) {
		// in-place is safe for the linear layout: element i is read and written by the same thread
		hipLaunchKernelGGL(dt_finish_kernel<0>, grid, dim3(256), 0, stream, work, dt, out);
	} else {
		hipLaunchKernelGGL(dt_finish_kernel<1>, grid, dim3(256), 0, stream, work, dt, out);
	}
	return hipGetLastError();
}

}  // namespace goicp
