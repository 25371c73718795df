// Stand-alone selftest of segment_plane_host (kdtree.cpp) for the sanitizer builds (make plane-asan / plane-tsan): host code
// only, its own main, no device.  The host function against a brute-force loop that restates the header -- every hypothesis of a round
// scored in turn on one thread, the first largest count kept, the moments summed in 128-bit integers without the split into words -- on
// small clouds (the sizes around a wave and a tile), on degenerate ones, and on 6 000 points x 1 000 hypotheses, where the host function
// scores blocks of hypotheses on several threads (from 2^20 pairs up).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "engine.hpp"

namespace {

int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

using goicp::PlaneRecord;
using goicp::PlaneSelect;

bool inl(const float* x, const float* a, const float* n, float d)
{
	const float e = ((x[0] - a[0]) * n[0] + (x[1] - a[1]) * n[1]) + (x[2] - a[2]) * n[2];
	return std::fabs(e) <= d;
}

void brute(const std::vector<float>& xyz, const PlaneSelect& s, std::vector<int32_t>* label, std::vector<PlaneRecord>* planes, std::vector<int32_t>* kept)
{
	const size_t n = xyz.size() / 3;
	label->assign(n, -1);
	planes->clear();
	std::vector<int32_t> map(n);
	for (size_t i = 0; i < n; i++) map[i] = (int32_t)i;
	for (int p = 0; p < s.max_planes; p++) {
		const size_t np = map.size();
		if (np < 3) break;
		auto pt = [&](size_t i) { return &xyz[3 * (size_t)map[i]]; };
		int best = -1, best_count = 0;
		float bn[3] = {0, 0, 0}, ba[3] = {0, 0, 0};
		for (int t = 0; t < s.iterations; t++) {
			uint32_t a, b, c;
			float nr[3] = {0.f, 0.f, 0.f};
			goicp::plane::draw(s.seed, (uint64_t)p * (uint64_t)s.iterations + (uint64_t)t, (uint32_t)np, &a, &b, &c);
			EXPECT(a != b && a != c && b != c && a < np && b < np && c < np);
			int count = 0;
			if (goicp::plane::of_triple(pt(a), pt(b), pt(c), nr))
				for (size_t i = 0; i < np; i++) count += inl(pt(i), pt(a), nr, s.distance) ? 1 : 0;
			if (best < 0 || count > best_count) {
				best = t; best_count = count;
				for (int k = 0; k < 3; k++) { bn[k] = nr[k]; ba[k] = pt(a)[k]; }
			}
		}
		if (best_count < std::max(s.min_inliers, 3)) break;
		PlaneRecord rec;
		for (int k = 0; k < 3; k++) { rec.normal[k] = bn[k]; rec.point[k] = ba[k]; }
		rec.inliers = best_count; rec.hypothesis = best; rec.refined = 0;
		if (s.refine) {
			float mn[3] = {INFINITY, INFINITY, INFINITY}, E = 0.f;
			for (size_t i = 0; i < np; i++) for (int k = 0; k < 3; k++) mn[k] = std::min(mn[k], pt(i)[k]);
			for (size_t i = 0; i < np; i++) for (int k = 0; k < 3; k++) E = std::max(E, pt(i)[k] - mn[k]);
			int e = 0;
			std::frexp(E, &e);
			unsigned __int128 m = 0, S[3] = {0, 0, 0}, P[6] = {0, 0, 0, 0, 0, 0};
			for (size_t i = 0; i < np; i++) {
				if (!inl(pt(i), ba, bn, s.distance)) continue;
				unsigned long long q[3];
				for (int k = 0; k < 3; k++) q[k] = (unsigned long long)std::llrint(std::ldexp((double)(pt(i)[k] - mn[k]), 31 - e));
				m++;
				int j = 0;
				for (int ka = 0; ka < 3; ka++) {
					S[ka] += q[ka];
					for (int kb = ka; kb < 3; kb++, j++) P[j] += (unsigned __int128)q[ka] * q[kb];
				}
			}
			// the words as the kernels would hand them over: any split of P with P = hi * 2^32 + lo gives the same finish
			unsigned long long w[goicp::kPlaneWords];
			w[0] = (unsigned long long)m;
			for (int k = 0; k < 3; k++) w[1 + k] = (unsigned long long)S[k];
			for (int j = 0; j < 6; j++) { w[4 + j] = (unsigned long long)(P[j] >> 32); w[10 + j] = (unsigned long long)(P[j] & 0xffffffffull); }
			float rn[3], rp[3];
			if (goicp::plane_refit(w, mn, e, rn, rp)) {
				int count = 0;
				for (size_t i = 0; i < np; i++) count += inl(pt(i), rp, rn, s.distance) ? 1 : 0;
				if (count >= rec.inliers) {
					for (int k = 0; k < 3; k++) { rec.normal[k] = rn[k]; rec.point[k] = rp[k]; }
					rec.inliers = count; rec.refined = 1;
				}
			}
		}
		rec.d = (float)-(((double)rec.normal[0] * (double)rec.point[0] + (double)rec.normal[1] * (double)rec.point[1]) + (double)rec.normal[2] * (double)rec.point[2]);
		std::vector<int32_t> next;
		for (size_t i = 0; i < np; i++) {
			if (inl(pt(i), rec.point, rec.normal, s.distance)) (*label)[(size_t)map[i]] = (int32_t)planes->size();
			else next.push_back(map[i]);
		}
		planes->push_back(rec);
		map.swap(next);
	}
	*kept = map;
}

void check(const std::vector<float>& xyz, float distance, int iterations, int refine, int max_planes, int min_inliers, uint64_t seed, int expect_planes = -1)
{
	const size_t n = xyz.size() / 3;
	const PlaneSelect s = goicp::plane_check_select(distance, iterations, refine, max_planes, min_inliers, seed);
	std::vector<int32_t> want_label, want_kept, label(n, -5), index(n, -5);
	std::vector<PlaneRecord> want_planes, planes((size_t)s.max_planes);
	std::vector<float> out(3 * n, -5.f);
	size_t c = 99, m = 99;
	brute(xyz, s, &want_label, &want_planes, &want_kept);
	goicp::plane_check_cloud(xyz.data(), n);
	goicp::segment_plane_host(xyz.data(), n, s, label.data(), out.data(), index.data(), planes.data(), &c, &m);
	EXPECT(c == want_planes.size() && m == want_kept.size());
	if (expect_planes >= 0) EXPECT(c == (size_t)expect_planes);
	if (c != want_planes.size() || m != want_kept.size()) return;
	EXPECT(label == want_label);
	for (size_t p = 0; p < c; p++) EXPECT(std::memcmp(&planes[p], &want_planes[p], sizeof(PlaneRecord)) == 0);
	for (size_t i = 0; i < m; i++) {
		EXPECT(index[i] == want_kept[i]);
		EXPECT(std::memcmp(&out[3 * i], &xyz[3 * (size_t)want_kept[i]], 3 * sizeof(float)) == 0);
	}
	for (size_t i = m; i < n; i++) EXPECT(index[i] == -5 && out[3 * i] == -5.f);
}

// a noisy tilted plane with a fifth of the points anywhere in the cube
std::vector<float> slab(size_t n, unsigned seed)
{
	std::mt19937 rng(seed);
	std::uniform_real_distribution<float> u(-1.f, 1.f);
	std::normal_distribution<float> g(0.f, 0.004f);
	std::vector<float> p(3 * n);
	for (size_t i = 0; i < n; i++) {
		p[3 * i] = u(rng); p[3 * i + 1] = u(rng);
		p[3 * i + 2] = i % 5 ? 0.3f * p[3 * i] - 0.2f * p[3 * i + 1] + g(rng) : u(rng);
	}
	return p;
}

}  // namespace

int main()
{
	for (size_t n : {3, 4, 63, 64, 65, 257, 1025})
		for (int T : {1, 63, 64, 65, 257})
			for (int refine : {0, 1}) check(slab(n, (unsigned)n), 0.012f, T, refine, 2, 0, 17 + (uint64_t)T);
	check(slab(1025, 2), 0.012f, 0, 1, 0, 0, 1);                                    // the defaults: 1 000 hypotheses, one plane
	check(slab(500, 3), 0.012f, 64, 1, 8, 300, 2, 1);                               // min_inliers above what the second round finds
	check(std::vector<float>(3 * 65, 0.25f), 0.01f, 65, 1, 1, 0, 0, 0);             // duplicates
	{
		std::vector<float> line(3 * 65);
		for (size_t i = 0; i < 65; i++) { line[3 * i] = (float)i; line[3 * i + 1] = 2.f * (float)i; line[3 * i + 2] = 3.f * (float)i; }
		check(line, 0.01f, 65, 1, 1, 0, 0, 0);                                       // collinear
	}
	check(slab(6000, 4), 0.012f, 1000, 1, 2, 0, 9);                                 // the threaded score: 6 000 x 1 000 pairs
	for (int bad = 0; bad < 6; bad++) {
		bool threw = false;
		try {
			goicp::plane_check_select(bad == 0 ? 0.f : 0.01f, bad == 1 ? -1 : (bad == 2 ? 65537 : 8), bad == 3 ? 2 : 1, bad == 4 ? 9 : 1, bad == 5 ? -1 : 0, 0);
		} catch (const std::invalid_argument&) { threw = true; }
		EXPECT(threw);
	}
	if (failures) { std::fprintf(stderr, "plane_selftest: %d failures\n", failures); return 1; }
	std::printf("plane_selftest ok\n");
	return 0;
}
