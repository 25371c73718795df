// Call sites of the FPFH descriptors and the descriptor matching in the C++ shim (include/goicp_mi355.hpp), compiled like
// tests/shim_normals.cpp: syntax-only by tests/test_fpfh_host.py, and as a program with -DSHIM_FPFH_MAIN by tests/test_gpu_fpfh.py, which
// runs it on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
using vec3 = Vec3;

// descriptors of a scan that is not the registration's source: normals towards the sensor, then FPFH over the k nearest other points
void describe(const icp::Registration& reg, const std::vector<vec3>& scan, int normal_k, int k, const float sensor[3], std::vector<float>& features,
              std::vector<uint8_t>* counts = nullptr)
{
	std::vector<vec3> normals;
	reg.estimate_normals(scan, scan.size(), normal_k, sensor, normals);
	reg.fpfh(scan, normals, scan.size(), k, features, counts);
}

// the mutual matches of two descriptor sets that pass the ratio test d2 <= ratio * d2_second
size_t mutual_matches(const icp::Registration& reg, const std::vector<float>& a, const std::vector<float>& b, float ratio, std::vector<int32_t>& index)
{
	std::vector<float> d2, second;
	std::vector<uint8_t> mutual;
	reg.match_features(a, b, index, d2, second, &mutual);
	size_t m = 0;
	for (size_t i = 0; i < index.size(); i++) m += mutual[i] && d2[i] <= ratio * second[i];
	return m;
}

#ifdef SHIM_FPFH_MAIN
// argv: model.f32 data.f32 k -- an engine on every 60th data point; the descriptors of every 7th and of every 9th data point on the device
// and their matches against the host functions (the same bits)
static std::vector<vec3> read_f32(const char* path, size_t stride)
{
	std::vector<vec3> out;
	FILE* f = std::fopen(path, "rb");
	if (!f) return out;
	float p[3];
	size_t i = 0;
	while (std::fread(p, sizeof(float), 3, f) == 3)
		if (i++ % stride == 0) out.push_back(vec3(p[0], p[1], p[2]));
	std::fclose(f);
	return out;
}

int main(int argc, char** argv)
{
	if (argc < 4) return 2;
	try {
		const int k = std::atoi(argv[3]);
		std::vector<vec3> model = read_f32(argv[1], 1), small = read_f32(argv[2], 60), a = read_f32(argv[2], 7), b = read_f32(argv[2], 9);
		if (model.empty() || small.empty() || a.size() < 64 || b.size() < 64) return 2;
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 64;
		icp::Registration reg(model, model.size(), small, small.size(), 1e-3f, &params);
		const float sensor[3] = {0.f, 0.f, 5.f};
		std::vector<float> fa, fb;
		std::vector<uint8_t> counts;
		describe(reg, a, 16, k, sensor, fa, &counts);
		describe(reg, b, 16, k, sensor, fb);
		std::vector<int32_t> index;
		const size_t m = mutual_matches(reg, fa, fb, 1.f, index);
		// the host functions on the same inputs
		bool same = true;
		const std::vector<vec3>* clouds[2] = {&a, &b};
		const std::vector<float>* feats[2] = {&fa, &fb};
		for (int c = 0; c < 2; c++) {
			const size_t n = clouds[c]->size();
			std::vector<float> nrm(3 * n), want(n * (size_t)GOICP_FPFH_DIM);
			check(goicp_estimate_normals_host(reinterpret_cast<const float*>(clouds[c]->data()), n, 16, sensor, nrm.data(), nullptr, nullptr));
			check(goicp_fpfh_host(reinterpret_cast<const float*>(clouds[c]->data()), nrm.data(), n, k, want.data(), nullptr));
			same = same && std::memcmp(want.data(), feats[c]->data(), sizeof(float) * want.size()) == 0;
		}
		std::vector<int32_t> hi(a.size());
		std::vector<float> hd(a.size()), hs(a.size());
		check(goicp_match_features_host(fa.data(), a.size(), fb.data(), b.size(), hi.data(), hd.data(), hs.data(), nullptr));
		same = same && hi == index;
		std::printf("%s: %zu and %zu points, k %d, %zu mutual matches\n", same ? "same bits" : "DIFFERENT", a.size(), b.size(), k, m);
		return same && m > 0 ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
