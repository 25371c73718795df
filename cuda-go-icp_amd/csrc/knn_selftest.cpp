// Stand-alone selftest of knn_self_host and estimate_normals_host (kdtree.cpp) for the sanitizer builds (make knn-asan /
// knn-tsan): host code only, its own main, no device.  The host functions against all pairs -- the k smallest keys (bits of d2) << 32 |
// index of a point by a plain scan over every other point, the normal by normal_pca_point on that row -- on small clouds of every shape the
// level search has a branch for, and on 66 000 points, where the level loops and the PCA run on several threads (from 65 536 points up), with
// the all-pairs scan on a sample of the points.
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

std::vector<uint64_t> keys_all_pairs(const std::vector<float>& p, size_t n, size_t i, int k)
{
	std::vector<uint64_t> keys;
	keys.reserve(n - 1);
	for (size_t j = 0; j < n; j++) {
		if (j == i) continue;
		const float dx = p[3 * i] - p[3 * j], dy = p[3 * i + 1] - p[3 * j + 1], dz = p[3 * i + 2] - p[3 * j + 2];
		const float d2 = dx * dx + dy * dy + dz * dz;
		uint32_t bits;
		std::memcpy(&bits, &d2, sizeof bits);
		keys.push_back(((uint64_t)bits << 32) | (uint32_t)j);
	}
	std::partial_sort(keys.begin(), keys.begin() + k, keys.end());
	keys.resize((size_t)k);
	return keys;
}

void check_cloud(const char* name, const std::vector<float>& p, int k, size_t sample)
{
	const size_t n = p.size() / 3;
	std::vector<int32_t> idx(n * (size_t)k);
	std::vector<float> d2(n * (size_t)k);
	goicp::knn_self_host(p.data(), n, k, idx.data(), d2.data());
	const size_t step = std::max<size_t>(1, n / std::max<size_t>(sample, 1));
	size_t bad = 0;
	for (size_t i = 0; i < n; i += step) {
		const std::vector<uint64_t> want = keys_all_pairs(p, n, i, k);
		for (int j = 0; j < k; j++) {
			uint32_t bits;
			std::memcpy(&bits, &d2[i * (size_t)k + (size_t)j], sizeof bits);
			if (want[(size_t)j] != (((uint64_t)bits << 32) | (uint32_t)idx[i * (size_t)k + (size_t)j])) { bad++; break; }
		}
	}
	if (bad) std::fprintf(stderr, "%s: k %d, %zu rows differ from all pairs\n", name, k, bad);
	EXPECT(bad == 0);
	if (k < 2) return;
	// the normals at k + 1 (the same rows), with and without a viewpoint
	const float vp[3] = {0.25f, -3.f, 7.f};
	for (int with_vp = 0; with_vp < 2; with_vp++) {
		std::vector<float> nrm(3 * n), var(n);
		std::vector<int32_t> used(n * (size_t)k);
		goicp::estimate_normals_host(p.data(), n, k + 1, with_vp ? vp : nullptr, nrm.data(), var.data(), used.data());
		EXPECT(used == idx);
		size_t wrong = 0;
		for (size_t i = 0; i < n; i += step) {
			float want_n[3], want_v;
			goicp::normal_pca_point(p.data(), (int)i, idx.data() + i * (size_t)k, k, with_vp != 0, vp[0], vp[1], vp[2], want_n, &want_v);
			if (std::memcmp(want_n, &nrm[3 * i], sizeof want_n) != 0 || std::memcmp(&want_v, &var[i], sizeof want_v) != 0) wrong++;
			const double len = std::sqrt((double)nrm[3 * i] * nrm[3 * i] + (double)nrm[3 * i + 1] * nrm[3 * i + 1] + (double)nrm[3 * i + 2] * nrm[3 * i + 2]);
			if (!(len == 0.0 || std::fabs(len - 1.0) <= 1.2e-7) || !(var[i] >= 0.f && var[i] <= 0.3333334f)) wrong++;
		}
		if (wrong) std::fprintf(stderr, "%s: k %d, %zu normals differ\n", name, k + 1, wrong);
		EXPECT(wrong == 0);
		// without the optional outputs
		std::vector<float> nrm2(3 * n);
		goicp::estimate_normals_host(p.data(), n, k + 1, with_vp ? vp : nullptr, nrm2.data(), nullptr, nullptr);
		EXPECT(std::memcmp(nrm.data(), nrm2.data(), sizeof(float) * 3 * n) == 0);
	}
}

template <class F> bool refuses(F&& call)
{
	try {
		call();
	} catch (const std::invalid_argument&) {
		return true;
	}
	return false;
}

}  // namespace

int main()
{
	std::mt19937 rng(12345);
	std::uniform_real_distribution<float> uni(-1.f, 1.f);
	auto uniform = [&](size_t n) { std::vector<float> p(3 * n); for (float& v : p) v = uni(rng); return p; };
	for (size_t n : {2u, 3u, 33u, 63u, 65u, 257u, 1000u, 4097u}) {
		const std::vector<float> p = uniform(n);
		for (int k : {1, 5, 16, 31})
			if ((size_t)k <= n - 1) check_cloud("uniform", p, k, 200);
		check_cloud("uniform", p, (int)std::min<size_t>(31, n - 1), 200);
	}
	{
		// identical points, duplicates, a plane, a unit lattice, denormal coordinates: no extent, ties, one flat axis, ties on every shell,
		// squares that underflow
		std::vector<float> same(3 * 300, 0.25f), base = uniform(40), dup, plane = uniform(500), lattice, den(3 * 200);
		for (int r = 0; r < 5; r++) dup.insert(dup.end(), base.begin(), base.end());
		for (size_t i = 0; i < 500; i++) plane[3 * i + 2] = 0.375f;
		for (int x = 0; x < 7; x++) for (int y = 0; y < 7; y++) for (int z = 0; z < 7; z++) { lattice.push_back((float)x); lattice.push_back((float)y); lattice.push_back((float)z); }
		for (float& v : den) v = std::ldexp((float)(int)(uni(rng) * 2000.f), -140);
		check_cloud("identical", same, 31, 300);
		check_cloud("duplicates", dup, 5, dup.size() / 3);
		check_cloud("planar", plane, 20, 500);
		check_cloud("lattice", lattice, 7, lattice.size() / 3);
		check_cloud("lattice", lattice, 19, lattice.size() / 3);
		check_cloud("denormal", den, 20, 200);
	}
	{
		// a cluster and points far from it: several levels, up to the radius that holds the cloud
		std::vector<float> p = uniform(2000);
		for (int i = 0; i < 30; i++) { p.push_back(10.f * std::pow(1.26f, (float)i) * (i % 2 ? 1.f : -1.f)); p.push_back(uni(rng)); p.push_back(uni(rng) * 100.f); }
		check_cloud("cluster", p, 20, p.size() / 3);
	}
	{
		// the threaded path: 66 000 points with 5 % spread wider, all pairs on a sample of 66 of them
		std::vector<float> p = uniform(66000);
		for (size_t i = 0; i < 66000; i += 20) for (int a = 0; a < 3; a++) p[3 * i + a] *= 3.f;
		check_cloud("threaded", p, 5, 66);
	}
	{
		const std::vector<float> p = uniform(16);
		std::vector<float> bad = p, nrm(48, -7.f), var(16, -7.f), d2(16 * 32, -7.f);
		std::vector<int32_t> idx(16 * 32, -7);
		bad[22] = NAN;
		const float nan_vp[3] = {0.f, NAN, 0.f}, inf_vp[3] = {INFINITY, 0.f, 0.f};
		auto knn = [&](const std::vector<float>& c, size_t n, int k) { return refuses([&] { goicp::knn_self_host(c.data(), n, k, idx.data(), d2.data()); }); };
		auto nor = [&](const std::vector<float>& c, size_t n, int k, const float* vp) {
			return refuses([&] { goicp::estimate_normals_host(c.data(), n, k, vp, nrm.data(), var.data(), idx.data()); });
		};
		EXPECT(knn(p, 16, 0) && knn(p, 16, -1) && knn(p, 16, 33) && knn(p, 16, 16) && knn(p, 1, 1) && knn(p, 0, 3) && knn(bad, 16, 3));
		EXPECT(nor(p, 16, 2, nullptr) && nor(p, 16, 33, nullptr) && nor(p, 16, 17, nullptr) && nor(p, 2, 3, nullptr) && nor(bad, 16, 3, nullptr));
		EXPECT(nor(p, 16, 3, nan_vp) && nor(p, 16, 3, inf_vp));
		EXPECT(refuses([&] { goicp::knn_self_host(p.data(), 16, 3, nullptr, d2.data()); }));
		EXPECT(refuses([&] { goicp::estimate_normals_host(p.data(), 16, 3, nullptr, nullptr, var.data(), idx.data()); }));
		bool untouched = true;
		for (float v : nrm) untouched = untouched && v == -7.f;
		for (float v : var) untouched = untouched && v == -7.f;
		for (float v : d2) untouched = untouched && v == -7.f;
		for (int32_t v : idx) untouched = untouched && v == -7;
		EXPECT(untouched);
	}
	if (failures) { std::fprintf(stderr, "knn selftest: %d failure(s)\n", failures); return 1; }
	std::printf("knn selftest ok\n");
	return 0;
}
