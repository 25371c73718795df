// Stand-alone selftest of ransac_pose_host and select_matches_host (kdtree.cpp) for the sanitizer builds (make ransac-asan /
// ransac-tsan): host code only, its own main, no device.  It checks the host function's control flow, not its arithmetic: the loop below
// calls the same device.hpp texts (plane::draw, pose::triple_ok, pose::of_triple) and the same ransac_pose_refit as the function under
// test, and differs in everything around them -- every hypothesis scored in turn on one thread, the poses picked by repeated search for
// the largest unused key, the moments summed in 128-bit integers without the split into words.  The independent restatement of the
// arithmetic is the numpy twin (tests/ransac_twin.py).  Inputs: the sizes around a wave, a tile and a workgroup's correspondences,
// degenerate ones, and 3 000 correspondences x 1 000 hypotheses, where the host function scores blocks of hypotheses on several threads
// (from 2^20 pairs up).
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

using goicp::RansacPoseFrame;
using goicp::RansacPoseRecord;
using goicp::RansacPoseSelect;

struct Input {
	std::vector<float> src, tgt;
	std::vector<int32_t> corr;
};

bool inl(const float* R, const float* t, const float* x, const float* m, float d2max)
{
	float e[3];
	for (int a = 0; a < 3; a++) e[a] = (((R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2]) + t[a]) - m[a];
	return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= d2max;
}

void brute(const Input& in, const RansacPoseSelect& s, std::vector<RansacPoseRecord>* poses, std::vector<uint8_t>* mask)
{
	const size_t M = in.corr.size() / 2;
	auto S = [&](size_t j) { return &in.src[3 * (size_t)in.corr[2 * j]]; };
	auto T = [&](size_t j) { return &in.tgt[3 * (size_t)in.corr[2 * j + 1]]; };
	const float d2max = s.distance * s.distance;
	auto hypothesis = [&](int t, float* R, float* tr) {
		uint32_t a, b, c;
		goicp::plane::draw(s.seed, (uint64_t)t, (uint32_t)M, &a, &b, &c);
		EXPECT(a != b && a != c && b != c && a < M && b < M && c < M);
		if (s.edge_similarity > 0.f && !goicp::pose::triple_ok(S(a), S(b), S(c), T(a), T(b), T(c), s.edge_similarity)) return false;
		return goicp::pose::of_triple(S(a), S(b), S(c), T(a), T(b), T(c), R, tr);
	};
	auto count_of = [&](const float* R, const float* tr) {
		int count = 0;
		for (size_t j = 0; j < M; j++) count += inl(R, tr, S(j), T(j), d2max) ? 1 : 0;
		return count;
	};
	std::vector<int> counts((size_t)s.iterations);
	for (int t = 0; t < s.iterations; t++) {
		float R[9], tr[3];
		counts[(size_t)t] = hypothesis(t, R, tr) ? count_of(R, tr) : 0;
	}
	std::vector<char> used((size_t)s.iterations, 0);
	poses->clear();
	for (int p = 0; p < s.max_poses && p < s.iterations; p++) {
		int best = -1;
		for (int t = 0; t < s.iterations; t++)
			if (!used[(size_t)t] && (best < 0 || counts[(size_t)t] > counts[(size_t)best])) best = t;   // the first largest
		if (counts[(size_t)best] < std::max(s.min_inliers, 3)) break;
		used[(size_t)best] = 1;
		RansacPoseRecord rec;
		EXPECT(hypothesis(best, rec.R, rec.t));
		rec.inliers = counts[(size_t)best]; rec.hypothesis = best; rec.refined = 0;
		if (s.refine) {
			RansacPoseFrame f[2];
			for (int side = 0; side < 2; side++) {
				float mn[3] = {INFINITY, INFINITY, INFINITY}, E = 0.f;
				for (size_t j = 0; j < M; j++) for (int k = 0; k < 3; k++) mn[k] = std::min(mn[k], (side ? T(j) : S(j))[k]);
				for (size_t j = 0; j < M; j++) for (int k = 0; k < 3; k++) E = std::max(E, (side ? T(j) : S(j))[k] - mn[k]);
				for (int k = 0; k < 3; k++) f[side].mn[k] = mn[k];
				std::frexp(E, &f[side].e);
			}
			unsigned __int128 m = 0, Ss[3] = {0, 0, 0}, St[3] = {0, 0, 0}, P[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
			for (size_t j = 0; j < M; j++) {
				if (!inl(rec.R, rec.t, S(j), T(j), d2max)) continue;
				unsigned long long qs[3], qt[3];
				for (int k = 0; k < 3; k++) {
					qs[k] = (unsigned long long)std::llrint(std::ldexp((double)(S(j)[k] - f[0].mn[k]), 31 - f[0].e));
					qt[k] = (unsigned long long)std::llrint(std::ldexp((double)(T(j)[k] - f[1].mn[k]), 31 - f[1].e));
				}
				m++;
				for (int a = 0; a < 3; a++) {
					Ss[a] += qs[a]; St[a] += qt[a];
					for (int b = 0; b < 3; b++) P[3 * a + b] += (unsigned __int128)qt[a] * qs[b];
				}
			}
			// the words as the kernels would hand them over: any split of P with P = hi * 2^32 + lo gives the same finish
			unsigned long long w[goicp::kRansacPoseWords];
			w[0] = (unsigned long long)m;
			for (int k = 0; k < 3; k++) { w[1 + k] = (unsigned long long)Ss[k]; w[4 + k] = (unsigned long long)St[k]; }
			for (int j = 0; j < 9; j++) { w[7 + j] = (unsigned long long)(P[j] >> 32); w[16 + j] = (unsigned long long)(P[j] & 0xffffffffull); }
			float R[9], tr[3];
			if (goicp::ransac_pose_refit(w, f[0], f[1], R, tr)) {
				const int count = count_of(R, tr);
				if (count >= rec.inliers) {
					std::memcpy(rec.R, R, sizeof(R)); std::memcpy(rec.t, tr, sizeof(tr));
					rec.inliers = count; rec.refined = 1;
				}
			}
		}
		poses->push_back(rec);
	}
	mask->assign(M, 0);
	if (!poses->empty())
		for (size_t j = 0; j < M; j++) (*mask)[j] = inl((*poses)[0].R, (*poses)[0].t, S(j), T(j), d2max) ? 1 : 0;
}

void check(const Input& in, float distance, int iterations, int refine, int max_poses, int min_inliers, float sigma, uint64_t seed, int expect_poses = -1)
{
	const size_t M = in.corr.size() / 2;
	const RansacPoseSelect s = goicp::ransac_pose_check_select(distance, iterations, refine, max_poses, min_inliers, sigma, seed);
	std::vector<RansacPoseRecord> want, poses((size_t)s.max_poses);
	std::vector<uint8_t> want_mask, mask(M, 9);
	size_t c = 99;
	brute(in, s, &want, &want_mask);
	goicp::ransac_pose_check_input(in.src.data(), in.src.size() / 3, in.tgt.data(), in.tgt.size() / 3, in.corr.data(), M);
	goicp::ransac_pose_host(in.src.data(), in.tgt.data(), in.corr.data(), M, s, poses.data(), &c, mask.data());
	EXPECT(c == want.size());
	if (expect_poses >= 0) EXPECT(c == (size_t)expect_poses);
	if (c != want.size()) return;
	for (size_t p = 0; p < c; p++) EXPECT(std::memcmp(&poses[p], &want[p], sizeof(RansacPoseRecord)) == 0);
	EXPECT(mask == want_mask);
}

// M correspondences between two clouds of M points: every second one pairs a point with its image under a fixed pose plus noise, the others
// pair it with some other point's image
Input scene(size_t M, unsigned seed, float offset = 0.f)
{
	std::mt19937 rng(seed);
	std::uniform_real_distribution<float> u(-1.f, 1.f);
	std::normal_distribution<float> g(0.f, 0.005f);
	Input in;
	in.src.resize(3 * M); in.tgt.resize(3 * M); in.corr.resize(2 * M);
	const float c = 0.6f, sn = 0.8f;
	for (size_t i = 0; i < M; i++) {
		const float x = u(rng), y = u(rng), z = u(rng);
		in.src[3 * i] = x + offset; in.src[3 * i + 1] = y + offset; in.src[3 * i + 2] = z + offset;
		in.tgt[3 * i] = c * x - sn * z + 0.3f + g(rng); in.tgt[3 * i + 1] = y - 0.2f + g(rng); in.tgt[3 * i + 2] = sn * x + c * z + 0.5f + g(rng);
		in.corr[2 * i] = (int32_t)i;
		in.corr[2 * i + 1] = (int32_t)(i % 2 == 0 || M <= 4 ? i : (i * 7 + 3) % M);
	}
	return in;
}

}  // namespace

int main()
{
	int i = 0;
	for (size_t M : {3, 4, 63, 64, 65, 1023, 1025})
		for (int T : {1, 63, 64, 65, 257})
			for (int refine : {0, 1}) {
				static const int K[3] = {1, 2, 64};
				static const float sg[3] = {0.f, 0.9f, 1.f};
				check(scene(M, (unsigned)M), 0.03f, T, refine, K[i % 3], 0, M > 4 ? sg[(i / 3) % 3] : 0.f, 17 + (uint64_t)T);
				i++;
			}
	check(scene(257, 5, 1000.f), 0.03f, 257, 1, 2, 0, 0.9f, 1);                    // the refit's frame: a coordinate offset of 1 000
	check(scene(257, 6), 0.03f, 65, 1, 1, 258, 0.9f, 0, 0);                        // min_inliers above M
	check(scene(257, 7), 0.03f, 257, 1, 64, 100, 0.f, 3);                          // more poses asked for than qualify
	{
		Input in = scene(65, 8);
		for (size_t j = 0; j < 65; j++) {                                          // collinear along an axis on both sides
			in.src[3 * j] = (float)j / 16.f; in.src[3 * j + 1] = in.src[3 * j + 2] = 0.f;
			in.tgt[3 * j] = in.tgt[3 * j + 1] = 0.f; in.tgt[3 * j + 2] = (float)j / 16.f;
			in.corr[2 * j + 1] = (int32_t)j;
		}
		check(in, 0.01f, 65, 1, 1, 0, 0.f, 0, 0);
		for (size_t j = 0; j < 65; j++) { in.src[3 * j] = 0.25f; in.src[3 * j + 1] = -0.5f; in.src[3 * j + 2] = 0.75f; }   // coincident source points
		check(in, 0.01f, 65, 1, 1, 0, 0.f, 0, 0);
	}
	{
		Input in = scene(129, 9);
		for (size_t j = 0; j < 129; j += 3) in.corr[2 * j] = in.corr[0];             // duplicated source indices
		check(in, 0.03f, 129, 1, 2, 0, 0.9f, 4);
	}
	check(scene(3000, 10), 0.03f, 1000, 1, 8, 0, 0.9f, 9);                         // the threaded score: 3 000 x 1 000 pairs
	for (int bad = 0; bad < 8; bad++) {
		bool threw = false;
		try {
			goicp::ransac_pose_check_select(bad == 0 ? 0.f : 0.01f, bad == 1 ? -1 : (bad == 2 ? (1 << 20) + 1 : 8), bad == 3 ? 2 : 1, bad == 4 ? 65 : 1, bad == 5 ? -1 : 0,
			                                bad == 6 ? 1.5f : (bad == 7 ? NAN : 0.9f), 0);
		} catch (const std::invalid_argument&) { threw = true; }
		EXPECT(threw);
	}
	{
		const Input in = scene(65, 11);
		for (int bad = 0; bad < 4; bad++) {
			Input b = in;
			if (bad == 0) b.corr[11] = 65;
			if (bad == 1) b.corr[10] = -1;
			if (bad == 2) b.src[7] = NAN;
			if (bad == 3) b.tgt[8] = INFINITY;
			bool threw = false;
			try {
				goicp::ransac_pose_check_input(b.src.data(), 65, b.tgt.data(), 65, b.corr.data(), 65);
			} catch (const std::invalid_argument&) { threw = true; }
			EXPECT(threw);
		}
	}
	{
		// select_matches against its statement
		const size_t n = 200;
		std::mt19937 rng(12);
		std::uniform_real_distribution<float> u(0.f, 1.f);
		std::vector<int32_t> index(n), corr(2 * n, -5);
		std::vector<float> d2(n), second(n);
		std::vector<uint8_t> mutual(n);
		for (size_t q = 0; q < n; q++) {
			index[q] = (int32_t)(rng() % 500); d2[q] = u(rng); second[q] = q % 7 ? d2[q] * (1.f + u(rng)) : INFINITY; mutual[q] = u(rng) < 0.6f;
		}
		for (float ratio : {0.f, 0.9f, 1.f})
			for (int req : {0, 1}) {
				size_t M = 99, want = 0;
				goicp::select_matches_host(index.data(), d2.data(), second.data(), req ? mutual.data() : nullptr, n, ratio, req, corr.data(), &M);
				const float rr = ratio * ratio;
				for (size_t q = 0; q < n; q++) {
					if ((req && !mutual[q]) || (ratio != 0.f && !(d2[q] <= rr * second[q]))) continue;
					EXPECT(want < M && corr[2 * want] == (int32_t)q && corr[2 * want + 1] == index[q]);
					want++;
				}
				EXPECT(M == want);
			}
	}
	if (failures) { std::fprintf(stderr, "ransac_selftest: %d failures\n", failures); return 1; }
	std::printf("ransac_selftest ok\n");
	return 0;
}
