// Stand-alone selftest of statistical_outlier_removal_host (kdtree.cpp) for the sanitizer builds (make stat-asan / stat-tsan):
// host code only, its own main, no device.  The host function against all pairs -- the k smallest d2 of a point by a plain scan over every
// other point, the sums and the finish restated from the header -- on small clouds of every shape the level search has a branch for, and on
// 66 000 points, where the level loops run on several threads (from 65 536 points up), with the all-pairs scan on a sample of the points.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "engine.hpp"

namespace {

int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

float u_all_pairs(const std::vector<float>& p, size_t n, size_t i, int k)
{
	std::vector<float> d2;
	d2.reserve(n - 1);
	for (size_t j = 0; j < n; j++) {
		if (j == i) continue;
		const float dx = p[3 * i] - p[3 * j], dy = p[3 * i + 1] - p[3 * j + 1], dz = p[3 * i + 2] - p[3 * j + 2];
		d2.push_back(dx * dx + dy * dy + dz * dz);
	}
	std::partial_sort(d2.begin(), d2.begin() + k, d2.end());
	double s = 0.0;
	for (int j = 0; j < k; j++) s += (double)std::sqrt(d2[(size_t)j]);
	return (float)(s / (double)k);
}

// the keep decisions and the threshold from u, as the header states them
void decide(const std::vector<float>& u, float alpha, std::vector<char>* keep, double* thr)
{
	const size_t n = u.size();
	keep->assign(n, 1);
	*thr = 0.0;
	const float U = *std::max_element(u.begin(), u.end());
	if (!(U > 0.f)) return;
	int e = 0;
	std::frexp(U, &e);
	std::vector<int64_t> q(n);
	int64_t S1 = 0, A = 0, B = 0;
	for (size_t i = 0; i < n; i++) {
		q[i] = (int64_t)std::floor(std::ldexp((double)u[i], 31 - e));
		S1 += q[i];
		A += (q[i] * q[i]) >> 32;
		B += (q[i] * q[i]) & 0xffffffffll;
	}
	const double nd = (double)n, mean = (double)S1 / nd, S2 = std::ldexp((double)A, 32) + (double)B;
	double var = (S2 - (double)S1 * mean) / (nd - 1.0);
	if (!(var > 0.0)) var = 0.0;
	const double Tq = mean + (double)alpha * std::sqrt(var);
	for (size_t i = 0; i < n; i++) (*keep)[i] = (double)q[i] <= Tq;
	*thr = std::ldexp(Tq, e - 31);
}

void check_cloud(const char* name, const std::vector<float>& p, int k, float alpha, size_t sample)
{
	const size_t n = p.size() / 3;
	std::vector<float> out(3 * n), u(n);
	std::vector<int32_t> idx(n);
	double thr = -1.0;
	size_t m = 0;
	goicp::statistical_outlier_removal_host(p.data(), n, k, alpha, out.data(), idx.data(), u.data(), &thr, &m);
	const size_t step = std::max<size_t>(1, n / std::max<size_t>(sample, 1));
	size_t bad = 0;
	for (size_t i = 0; i < n; i += step) {
		const float want = u_all_pairs(p, n, i, k);
		if (std::memcmp(&want, &u[i], sizeof(float)) != 0) bad++;
	}
	if (bad) std::fprintf(stderr, "%s: k %d, %zu mean distances differ from all pairs\n", name, k, bad);
	EXPECT(bad == 0);
	std::vector<char> keep;
	double want_thr = 0.0;
	decide(u, alpha, &keep, &want_thr);
	EXPECT(std::memcmp(&thr, &want_thr, sizeof(double)) == 0);
	size_t w = 0;
	bool same = true;
	for (size_t i = 0; i < n; i++) {
		if (!keep[i]) continue;
		same = same && w < m && idx[w] == (int32_t)i && std::memcmp(&out[3 * w], &p[3 * i], 3 * sizeof(float)) == 0;
		w++;
	}
	EXPECT(same && w == m && m >= 1);
}

bool refuses(const std::vector<float>& p, size_t n, int k, float alpha)
{
	std::vector<float> out(3 * std::max<size_t>(n, 1), -7.f), u(std::max<size_t>(n, 1), -7.f);
	std::vector<int32_t> idx(std::max<size_t>(n, 1), -7);
	double thr = -7.0;
	size_t m = 99;
	try {
		goicp::statistical_outlier_removal_host(p.data(), n, k, alpha, out.data(), idx.data(), u.data(), &thr, &m);
	} catch (const std::invalid_argument&) {
		bool untouched = thr == -7.0 && m == 99;
		for (float v : out) untouched = untouched && v == -7.f;
		for (float v : u) untouched = untouched && v == -7.f;
		for (int32_t v : idx) untouched = untouched && v == -7;
		return untouched;
	}
	return false;
}

}  // namespace

int main()
{
	std::mt19937 rng(12345);
	std::uniform_real_distribution<float> uni(-1.f, 1.f);
	auto uniform = [&](size_t n) { std::vector<float> p(3 * n); for (float& v : p) v = uni(rng); return p; };
	for (size_t n : {2u, 3u, 63u, 65u, 257u, 1000u, 4097u}) {
		const std::vector<float> p = uniform(n);
		for (int k : {1, 5, 20, 64})
			if ((size_t)k <= n - 1) check_cloud("uniform", p, k, 1.f, 200);
		check_cloud("uniform", p, (int)std::min<size_t>(64, n - 1), 0.f, 200);
	}
	{
		// identical points, duplicates, a plane, denormal coordinates: no extent, ties, one flat axis, squares that underflow
		std::vector<float> same(3 * 300, 0.25f), base = uniform(40), dup, plane = uniform(500), den(3 * 200);
		for (int r = 0; r < 5; r++) dup.insert(dup.end(), base.begin(), base.end());
		for (size_t i = 0; i < 500; i++) plane[3 * i + 2] = 0.375f;
		for (float& v : den) v = std::ldexp((float)(int)(uni(rng) * 2000.f), -140);
		check_cloud("identical", same, 64, 2.f, 300);
		check_cloud("duplicates", dup, 5, 1.f, dup.size() / 3);
		check_cloud("planar", plane, 20, 2.f, 500);
		check_cloud("denormal", den, 20, 2.f, 200);
	}
	{
		// a cluster and points far from it: several levels, up to the radius that holds the cloud
		std::vector<float> p = uniform(2000);
		for (int i = 0; i < 30; i++) { p.push_back(10.f * std::pow(1.26f, (float)i) * (i % 2 ? 1.f : -1.f)); p.push_back(uni(rng)); p.push_back(uni(rng) * 100.f); }
		check_cloud("cluster", p, 20, 2.f, p.size() / 3);
	}
	{
		// the threaded path: 66 000 points with 5 % spread wider, all pairs on a sample of 66 of them
		std::vector<float> p = uniform(66000);
		for (size_t i = 0; i < 66000; i += 20) for (int a = 0; a < 3; a++) p[3 * i + a] *= 3.f;
		check_cloud("threaded", p, 5, 2.f, 66);
	}
	{
		const std::vector<float> p = uniform(16);
		std::vector<float> bad = p;
		bad[22] = NAN;
		EXPECT(refuses(p, 16, 0, 1.f) && refuses(p, 16, -1, 1.f) && refuses(p, 16, 65, 1.f) && refuses(p, 16, 16, 1.f) && refuses(p, 1, 1, 1.f));
		EXPECT(refuses(p, 16, 3, -1.f) && refuses(p, 16, 3, NAN) && refuses(p, 16, 3, INFINITY) && refuses(bad, 16, 3, 1.f) && refuses(p, 0, 3, 1.f));
	}
	if (failures) { std::fprintf(stderr, "stat selftest: %d failure(s)\n", failures); return 1; }
	std::printf("stat selftest ok\n");
	return 0;
}
