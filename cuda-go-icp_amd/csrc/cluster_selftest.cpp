// Stand-alone selftest of cluster_host / cluster_filter_host (kdtree.cpp) for the sanitizer builds (make cluster-asan /
// cluster-tsan, and part of make asan): host code only, its own main, no device.  The host functions against all pairs -- the neighbour
// lists by a plain scan over every other point, the components by a breadth-first walk over the core points, the border points by the
// smallest key, the selection restated from the header -- on small clouds of every shape the grid has a branch for, and on 66 000 points,
// where the core count runs on several threads (from 65 536 points up), against a walk that takes its neighbours from a coarse sort.
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

float pair_d2(const std::vector<float>& p, size_t i, size_t j)
{
	const float dx = p[3 * i] - p[3 * j], dy = p[3 * i + 1] - p[3 * j + 1], dz = p[3 * i + 2] - p[3 * j + 2];
	return dx * dx + dy * dy + dz * dz;
}

// labels and sizes from neighbour lists, as the header states them
void label_from_lists(const std::vector<float>& p, const std::vector<std::vector<int32_t>>& nb, int k, std::vector<int32_t>* label, std::vector<int32_t>* sizes)
{
	const size_t n = nb.size();
	std::vector<char> core(n);
	for (size_t i = 0; i < n; i++) core[i] = std::min<size_t>(nb[i].size(), (size_t)k) == (size_t)k;
	label->assign(n, -1);
	sizes->clear();
	for (size_t i = 0; i < n; i++) {
		if (!core[i] || (*label)[i] >= 0) continue;            // ascending i: a new cluster starts at its smallest core index
		const int32_t l = (int32_t)sizes->size();
		sizes->push_back(0);
		std::vector<int32_t> todo{(int32_t)i};
		(*label)[i] = l;
		while (!todo.empty()) {
			const int32_t a = todo.back();
			todo.pop_back();
			(*sizes)[(size_t)l]++;
			for (int32_t b : nb[(size_t)a])
				if (core[(size_t)b] && (*label)[(size_t)b] < 0) { (*label)[(size_t)b] = l; todo.push_back(b); }
		}
	}
	for (size_t i = 0; i < n; i++) {
		if (core[i]) continue;
		uint64_t best = UINT64_MAX;
		for (int32_t b : nb[i]) {
			if (!core[(size_t)b]) continue;
			const float d2 = pair_d2(p, i, (size_t)b);
			uint32_t bits;
			std::memcpy(&bits, &d2, sizeof(bits));
			best = std::min(best, ((uint64_t)bits << 32) | (uint64_t)(uint32_t)b);
		}
		if (best == UINT64_MAX) continue;
		(*label)[i] = (*label)[(size_t)(best & 0xffffffffu)];
		(*sizes)[(size_t)(*label)[i]]++;
	}
}

std::vector<std::vector<int32_t>> lists_all_pairs(const std::vector<float>& p, float r)
{
	const size_t n = p.size() / 3;
	const float r2 = r * r;
	std::vector<std::vector<int32_t>> nb(n);
	for (size_t i = 0; i < n; i++)
		for (size_t j = 0; j < n; j++)
			if (j != i && pair_d2(p, i, j) <= r2) nb[i].push_back((int32_t)j);
	return nb;
}

// for the large cloud: the points sorted by x, a window of +- r around every point
std::vector<std::vector<int32_t>> lists_sorted_x(const std::vector<float>& p, float r)
{
	const size_t n = p.size() / 3;
	const float r2 = r * r;
	std::vector<int32_t> order(n);
	for (size_t i = 0; i < n; i++) order[i] = (int32_t)i;
	std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return p[3 * (size_t)a] < p[3 * (size_t)b]; });
	std::vector<std::vector<int32_t>> nb(n);
	for (size_t s = 0; s < n; s++) {
		const size_t i = (size_t)order[s];
		for (size_t t = s + 1; t < n && p[3 * (size_t)order[t]] - p[3 * i] <= r * 1.001f; t++) {
			const size_t j = (size_t)order[t];
			if (pair_d2(p, i, j) <= r2) { nb[i].push_back((int32_t)j); nb[j].push_back((int32_t)i); }
		}
	}
	return nb;
}

void check_cloud(const char* name, const std::vector<float>& p, float r, int k, bool all_pairs = true)
{
	const size_t n = p.size() / 3;
	std::vector<int32_t> want, wsizes, label(n), sizes(n);
	label_from_lists(p, all_pairs ? lists_all_pairs(p, r) : lists_sorted_x(p, r), k, &want, &wsizes);
	size_t c = 0;
	goicp::cluster_host(p.data(), n, r, k, label.data(), sizes.data(), &c);
	sizes.resize(c);
	if (label != want || sizes != wsizes) std::fprintf(stderr, "%s: r %g k %d: %zu clusters, wanted %zu\n", name, r, k, c, wsizes.size());
	EXPECT(label == want && sizes == wsizes);
	// the selection: the two largest clusters of at least 3 points, restated
	std::vector<int32_t> order(c);
	for (size_t l = 0; l < c; l++) order[l] = (int32_t)l;
	std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return wsizes[(size_t)a] > wsizes[(size_t)b]; });
	std::vector<char> keep(c, 0);
	for (size_t q = 0; q < std::min<size_t>(2, c); q++) keep[(size_t)order[q]] = wsizes[(size_t)order[q]] >= 3;
	std::vector<float> out(3 * n);
	std::vector<int32_t> idx(n), lab(n);
	size_t m = 0;
	goicp::cluster_filter_host(p.data(), n, r, k, 3, 2, out.data(), idx.data(), lab.data(), &m);
	size_t w = 0;
	bool same = true;
	for (size_t i = 0; i < n; i++) {
		if (want[i] < 0 || !keep[(size_t)want[i]]) continue;
		same = same && w < m && idx[w] == (int32_t)i && lab[w] == want[i] && std::memcmp(&out[3 * w], &p[3 * i], 3 * sizeof(float)) == 0;
		w++;
	}
	EXPECT(same && w == m);
}

bool refuses(const std::vector<float>& p, size_t n, float r, int k, int min_size = 0, int max_clusters = 0)
{
	const size_t room = std::max<size_t>(n, 1);
	std::vector<float> out(3 * room, -7.f);
	std::vector<int32_t> label(room, -7), sizes(room, -7), idx(room, -7);
	size_t c = 99, m = 99;
	int thrown = 0;
	try { goicp::cluster_host(p.data(), n, r, k, label.data(), sizes.data(), &c); } catch (const std::invalid_argument&) { thrown++; }
	try { goicp::cluster_filter_host(p.data(), n, r, k, min_size, max_clusters, out.data(), idx.data(), label.data(), &m); } catch (const std::invalid_argument&) { thrown++; }
	bool untouched = m == 99 && (c == 99 || (min_size < 0 || max_clusters < 0));       // a bad selection is the filter's refusal alone
	for (float v : out) untouched = untouched && v == -7.f;
	for (int32_t v : idx) untouched = untouched && v == -7;
	return untouched && thrown >= 1 && (thrown == 2 || min_size < 0 || max_clusters < 0);
}

}  // namespace

int main()
{
	std::mt19937 rng(4321);
	std::uniform_real_distribution<float> uni(0.f, 1.f);
	auto uniform = [&](size_t n, float lo = 0.f, float hi = 1.f) { std::vector<float> p(3 * n); for (float& v : p) v = lo + (hi - lo) * uni(rng); return p; };
	for (size_t n : {1u, 2u, 3u, 255u, 256u, 257u, 1023u, 1025u}) {
		const std::vector<float> p = uniform(n);
		const float s = std::cbrt(1.f / (float)n);
		for (float r : {0.7f * s, 1.2f * s, 4.f})
			for (int k : {0, 1, 3, 1000}) check_cloud("uniform", p, r, k);
	}
	{
		// identical points, duplicates, a plane, an offset cloud, negative coordinates, a chain
		std::vector<float> same(3 * 300, 0.25f), base = uniform(60), dup, plane = uniform(500), off = uniform(600, 999.99f, 1000.01f), neg = uniform(500, -1.f, -0.5f), chain;
		for (int q = 0; q < 5; q++) dup.insert(dup.end(), base.begin(), base.end());
		for (size_t i = 0; i < 500; i++) plane[3 * i + 2] = 0.375f;
		for (int i = 0; i < 2048; i++) { chain.push_back(0.9f * (float)((i * 1237) % 2048)); chain.push_back(0.f); chain.push_back(0.f); }
		for (int k : {0, 2, 299}) check_cloud("identical", same, 0.5f, k);
		for (int k : {0, 4, 5}) check_cloud("duplicates", dup, 0.05f, k);
		for (int k : {0, 3}) check_cloud("planar", plane, 0.06f, k);
		for (int k : {0, 2}) check_cloud("offset", off, 0.002f, k);
		for (int k : {0, 2}) check_cloud("negative", neg, 0.05f, k);
		for (int k : {0, 2, 3}) check_cloud("chain", chain, 1.f, k);
	}
	{
		// the threaded path: 66 000 points
		const std::vector<float> p = uniform(66000);
		check_cloud("threaded", p, 0.02f, 3, false);
		check_cloud("threaded", p, 0.015f, 0, false);
	}
	{
		const std::vector<float> p = uniform(16);
		std::vector<float> bad = p;
		bad[22] = NAN;
		EXPECT(refuses(p, 16, 0.f, 1) && refuses(p, 16, -1.f, 1) && refuses(p, 16, NAN, 1) && refuses(p, 16, INFINITY, 1) && refuses(p, 16, 1e-25f, 1));
		EXPECT(refuses(p, 16, 1e25f, 1) && refuses(p, 16, 1e-6f, 1) && refuses(p, 16, 0.5f, -1) && refuses(bad, 16, 0.5f, 1) && refuses(p, 0, 0.5f, 1));
		EXPECT(refuses(p, 16, 0.5f, 1, -1, 0) && refuses(p, 16, 0.5f, 1, 0, -1));
	}
	if (failures) { std::fprintf(stderr, "cluster selftest: %d failure(s)\n", failures); return 1; }
	std::printf("cluster selftest ok\n");
	return 0;
}
