// Stand-alone selftest of fpfh_host and match_features_host (kdtree.cpp) for the sanitizer builds (make fpfh-asan / fpfh-tsan):
// host code only, its own main, no device.  The host functions against an all-pairs restatement -- the row of a point by a plain scan over
// every other point, its counts by fpfh::pair_bins over that row, its descriptor bin by bin over the rows of its neighbours, the nearest
// descriptor by a plain scan with a sort of all keys -- on small clouds (duplicates, zero normals, a normal along the offset, a lattice)
// and on 66 000 points, where the level loops, the two descriptor passes and the matcher run on several threads, with the restatement on a
// sample of the points.
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
constexpr int D = goicp::kFpfhDim;

uint64_t key_of(float d2, size_t j)
{
	uint32_t bits;
	std::memcpy(&bits, &d2, sizeof bits);
	return ((uint64_t)bits << 32) | (uint32_t)j;
}

float d2_of(uint64_t key)
{
	const uint32_t bits = (uint32_t)(key >> 32);
	float d2;
	std::memcpy(&d2, &bits, sizeof d2);
	return d2;
}

std::vector<uint64_t> row_all_pairs(const std::vector<float>& p, size_t n, size_t i, int k)
{
	std::vector<uint64_t> keys;
	for (size_t j = 0; j < n; j++) {
		if (j == i) continue;
		const float dx = p[3 * i] - p[3 * j], dy = p[3 * i + 1] - p[3 * j + 1], dz = p[3 * i + 2] - p[3 * j + 2];
		keys.push_back(key_of(dx * dx + dy * dy + dz * dz, j));
	}
	std::partial_sort(keys.begin(), keys.begin() + k, keys.end());
	keys.resize((size_t)k);
	return keys;
}

std::vector<int> counts_all_pairs(const std::vector<float>& p, const std::vector<float>& nrm, size_t n, size_t i, int k)
{
	std::vector<int> c((size_t)D, 0);
	for (uint64_t key : row_all_pairs(p, n, i, k)) {
		const size_t j = (size_t)(key & 0xffffffffull);
		int b[3];
		if (!goicp::fpfh::pair_bins(&p[3 * i], &nrm[3 * i], &p[3 * j], &nrm[3 * j], b)) continue;
		c[(size_t)b[0]]++; c[(size_t)(11 + b[1])]++; c[(size_t)(22 + b[2])]++;
	}
	return c;
}

void check_cloud(const char* name, const std::vector<float>& p, const std::vector<float>& nrm, int k, size_t sample)
{
	const size_t n = p.size() / 3;
	std::vector<float> out(n * (size_t)D), out2(n * (size_t)D);
	std::vector<uint8_t> cnt(n * (size_t)D);
	goicp::fpfh_host(p.data(), nrm.data(), n, k, out.data(), cnt.data());
	goicp::fpfh_host(p.data(), nrm.data(), n, k, out2.data(), nullptr);
	EXPECT(std::memcmp(out.data(), out2.data(), sizeof(float) * out.size()) == 0);
	const size_t step = std::max<size_t>(1, n / std::max<size_t>(sample, 1));
	const double inc = 100.0 / (double)k;
	size_t bad = 0;
	for (size_t i = 0; i < n; i += step) {
		const std::vector<int> own = counts_all_pairs(p, nrm, n, i, k);
		const std::vector<uint64_t> row = row_all_pairs(p, n, i, k);
		std::vector<std::vector<int>> theirs;
		for (uint64_t key : row) theirs.push_back(counts_all_pairs(p, nrm, n, (size_t)(key & 0xffffffffull), k));
		bool same = true;
		for (int g = 0; g < 3 && same; g++) {
			double a[11], s = 0.0;
			for (int b = 0; b < 11; b++) {
				a[b] = 0.0;
				for (size_t j = 0; j < row.size(); j++) {
					const float w2 = d2_of(row[j]);
					if (w2 == 0.f) continue;
					a[b] = a[b] + ((double)theirs[j][(size_t)(11 * g + b)] * inc) * (1.0 / (double)w2);
				}
				s = s + a[b];
			}
			for (int b = 0; b < 11; b++) {
				const double v = s > 0.0 ? a[b] * (100.0 / s) : a[b];
				const float want = (float)(v + (double)own[(size_t)(11 * g + b)] * inc);
				same = same && std::memcmp(&want, &out[i * D + (size_t)(11 * g + b)], sizeof want) == 0 && cnt[i * D + (size_t)(11 * g + b)] == own[(size_t)(11 * g + b)];
			}
		}
		bad += !same;
	}
	if (bad) std::fprintf(stderr, "%s: k %d, %zu descriptors differ from the restatement\n", name, k, bad);
	EXPECT(bad == 0);
}

void check_match(const char* name, const std::vector<float>& q, const std::vector<float>& t, size_t sample)
{
	const size_t nq = q.size() / D, nt = t.size() / D;
	std::vector<int32_t> idx(nq), idx2(nq);
	std::vector<float> d2(nq), second(nq), d2b(nq), secondb(nq);
	std::vector<uint8_t> mutual(nq);
	goicp::match_features_host(q.data(), nq, t.data(), nt, idx.data(), d2.data(), second.data(), mutual.data());
	goicp::match_features_host(q.data(), nq, t.data(), nt, idx2.data(), d2b.data(), secondb.data(), nullptr);
	EXPECT(idx == idx2 && std::memcmp(d2.data(), d2b.data(), sizeof(float) * nq) == 0 && std::memcmp(second.data(), secondb.data(), sizeof(float) * nq) == 0);
	auto sorted_keys = [](const float* a, const std::vector<float>& set, size_t m) {
		std::vector<uint64_t> keys;
		for (size_t j = 0; j < m; j++) {
			float s = 0.f;
			for (int c = 0; c < D; c++) { const float d = a[c] - set[j * D + (size_t)c]; s = s + d * d; }
			keys.push_back(key_of(s, j));
		}
		std::sort(keys.begin(), keys.end());
		return keys;
	};
	const size_t step = std::max<size_t>(1, nq / std::max<size_t>(sample, 1));
	size_t bad = 0;
	for (size_t i = 0; i < nq; i += step) {
		const std::vector<uint64_t> keys = sorted_keys(&q[i * D], t, nt);
		const size_t j = (size_t)(keys[0] & 0xffffffffull);
		const float want_d2 = d2_of(keys[0]), want_second = nt > 1 ? d2_of(keys[1]) : INFINITY;
		const bool back = (sorted_keys(&t[j * D], q, nq)[0] & 0xffffffffull) == i;
		if ((size_t)idx[i] != j || std::memcmp(&d2[i], &want_d2, sizeof(float)) != 0 ||
		    std::memcmp(&second[i], &want_second, sizeof(float)) != 0 || mutual[i] != (back ? 1 : 0))
			bad++;
	}
	if (bad) std::fprintf(stderr, "%s: %zu x %zu, %zu matches differ from the restatement\n", name, nq, nt, bad);
	EXPECT(bad == 0);
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
	std::mt19937 rng(4321);
	std::uniform_real_distribution<float> uni(-1.f, 1.f);
	auto uniform = [&](size_t n) { std::vector<float> p(3 * n); for (float& v : p) v = uni(rng); return p; };
	auto unit = [&](size_t n) {
		std::vector<float> v = uniform(n);
		for (size_t i = 0; i < n; i++) {
			const float l = std::sqrt(v[3 * i] * v[3 * i] + v[3 * i + 1] * v[3 * i + 1] + v[3 * i + 2] * v[3 * i + 2]);
			for (int a = 0; a < 3; a++) v[3 * i + a] = l > 0.f ? v[3 * i + a] / l : (a == 2 ? 1.f : 0.f);
		}
		return v;
	};
	for (size_t n : {2u, 3u, 33u, 65u, 257u, 1000u})
		for (int k : {1, 2, 16, 32})
			if ((size_t)k <= n - 1) check_cloud("uniform", uniform(n), unit(n), k, 100);
	{
		// duplicates (d2 == 0), zero normals, a normal along the offset (vl2 == 0), a lattice with axis normals (every feature on a bin edge)
		std::vector<float> base = uniform(40), dup, dn = unit(40), dupn, lattice, ln;
		for (int r = 0; r < 4; r++) { dup.insert(dup.end(), base.begin(), base.end()); dupn.insert(dupn.end(), dn.begin(), dn.end()); }
		for (size_t i = 0; i < 160; i += 7) dupn[3 * i] = dupn[3 * i + 1] = dupn[3 * i + 2] = 0.f;
		check_cloud("duplicates", dup, dupn, 8, 160);
		for (int x = 0; x < 6; x++) for (int y = 0; y < 6; y++) for (int z = 0; z < 6; z++) {
			lattice.push_back((float)x); lattice.push_back((float)y); lattice.push_back((float)z);
			const int a = (x + 2 * y + 3 * z) % 3;
			for (int c = 0; c < 3; c++) ln.push_back(c == a ? ((x + y + z) % 2 ? -1.f : 1.f) : 0.f);
		}
		check_cloud("lattice", lattice, ln, 6, 216);
		check_cloud("lattice", lattice, ln, 26, 216);
	}
	{
		// the threaded path: 66 000 points, the restatement on a sample of 40 of them
		check_cloud("threaded", uniform(66000), unit(66000), 5, 40);
	}
	{
		auto descriptors = [&](size_t n) { std::vector<float> f(n * D); for (float& v : f) v = 50.f * (uni(rng) + 1.f); return f; };
		for (size_t nq : {1u, 2u, 65u, 257u})
			for (size_t nt : {1u, 2u, 64u, 300u}) check_match("uniform", descriptors(nq), descriptors(nt), 300);
		std::vector<float> t = descriptors(50), q = descriptors(70);
		for (int r = 0; r < 25; r++) std::memcpy(&t[(size_t)(25 + r) * D], &t[(size_t)r * D], sizeof(float) * D);   // every target twice
		std::memcpy(&q[0], &t[3 * D], sizeof(float) * D);
		check_match("ties", q, t, 70);
		check_match("identical", std::vector<float>(40 * D, 1.5f), std::vector<float>(30 * D, 1.5f), 40);
		check_match("threaded", descriptors(3000), descriptors(2500), 50);
	}
	{
		const std::vector<float> p = uniform(16), nrm = unit(16), f(16 * D, 1.f);
		std::vector<float> bad = p, badn = nrm, badf = f, out(16 * D, -7.f), d2(16, -7.f), second(16, -7.f);
		std::vector<uint8_t> cnt(16 * D, 7), mutual(16, 7);
		std::vector<int32_t> idx(16, -7);
		bad[22] = NAN; badn[5] = INFINITY; badf[40] = NAN;
		auto fp = [&](const std::vector<float>& c, const float* m, size_t n, int k) { return refuses([&] { goicp::fpfh_host(c.data(), m, n, k, out.data(), cnt.data()); }); };
		auto ma = [&](const float* q, size_t nq, const float* t, size_t nt) {
			return refuses([&] { goicp::match_features_host(q, nq, t, nt, idx.data(), d2.data(), second.data(), mutual.data()); });
		};
		EXPECT(fp(p, nrm.data(), 16, 0) && fp(p, nrm.data(), 16, 33) && fp(p, nrm.data(), 16, 16) && fp(p, nrm.data(), 1, 1) && fp(p, nrm.data(), 0, 3));
		EXPECT(fp(bad, nrm.data(), 16, 3) && fp(p, badn.data(), 16, 3) && fp(p, nullptr, 16, 3));
		EXPECT(refuses([&] { goicp::fpfh_host(p.data(), nrm.data(), 16, 3, nullptr, cnt.data()); }));
		EXPECT(ma(nullptr, 16, f.data(), 16) && ma(f.data(), 16, nullptr, 16) && ma(f.data(), 0, f.data(), 16) && ma(f.data(), 16, f.data(), 0));
		EXPECT(ma(badf.data(), 16, f.data(), 16) && ma(f.data(), 16, badf.data(), 16) && ma(f.data(), (size_t)1 << 40, f.data(), 16));
		EXPECT(refuses([&] { goicp::match_features_host(f.data(), 16, f.data(), 16, nullptr, d2.data(), second.data(), nullptr); }));
		bool untouched = true;
		for (float v : out) untouched = untouched && v == -7.f;
		for (float v : d2) untouched = untouched && v == -7.f;
		for (float v : second) untouched = untouched && v == -7.f;
		for (uint8_t v : cnt) untouched = untouched && v == 7;
		for (uint8_t v : mutual) untouched = untouched && v == 7;
		for (int32_t v : idx) untouched = untouched && v == -7;
		EXPECT(untouched);
	}
	if (failures) { std::fprintf(stderr, "fpfh selftest: %d failure(s)\n", failures); return 1; }
	std::printf("fpfh selftest ok\n");
	return 0;
}
