// Call sites of the self k-NN and the normal estimation in the C++ shim (include/goicp_mi355.hpp), compiled like tests/shim_stat_outlier.cpp:
// syntax-only by tests/test_normals_host.py, and as a program with -DSHIM_NORMALS_MAIN by tests/test_gpu_normals.py, which runs it on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
using vec3 = Vec3;

// normals of a scan that is not the registration's source, towards the sensor; the share of points flatter than `flat`
float flat_share(const icp::Registration& reg, const std::vector<vec3>& scan, int k, const float sensor[3], float flat, std::vector<vec3>& normals)
{
	std::vector<float> variation;
	reg.estimate_normals(scan, scan.size(), k, sensor, normals, &variation);
	size_t m = 0;
	for (float v : variation) m += v <= flat;
	return (float)m / (float)scan.size();
}

// the neighbours of every point, and the largest distance to a k-th neighbour
float widest_neighbourhood(const icp::Registration& reg, const std::vector<vec3>& scan, int k, std::vector<int32_t>& index)
{
	std::vector<float> d2;
	reg.knn_self(scan, scan.size(), k, index, &d2);
	float w = 0.f;
	for (size_t i = 0; i < scan.size(); i++) w = d2[i * (size_t)k + (size_t)k - 1] > w ? d2[i * (size_t)k + (size_t)k - 1] : w;
	return w;
}

#ifdef SHIM_NORMALS_MAIN
// argv: model.f32 data.f32 k -- an engine on every 60th data point; the normals and the neighbours of every 3rd data point on the device
// against the host functions (the same bits)
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
		std::vector<vec3> model = read_f32(argv[1], 1), small = read_f32(argv[2], 60), scan = read_f32(argv[2], 3);
		if (model.empty() || small.empty() || scan.size() < 64) return 2;
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 64;
		icp::Registration reg(model, model.size(), small, small.size(), 1e-3f, &params);
		const float sensor[3] = {0.f, 0.f, 5.f};
		const size_t n = scan.size();
		std::vector<vec3> normals;
		std::vector<int32_t> index;
		const float share = flat_share(reg, scan, k, sensor, 0.05f, normals);
		const float widest = widest_neighbourhood(reg, scan, k - 1, index);
		std::vector<float> host_n(3 * n), host_v(n);
		std::vector<int32_t> host_i(n * (size_t)(k - 1));
		check(goicp_estimate_normals_host(reinterpret_cast<const float*>(scan.data()), n, k, sensor, host_n.data(), host_v.data(), host_i.data()));
		const bool same = std::memcmp(host_n.data(), normals.data(), sizeof(float) * 3 * n) == 0 && index.size() == host_i.size() &&
		                  std::memcmp(host_i.data(), index.data(), sizeof(int32_t) * index.size()) == 0;
		std::printf("%s: %zu points, k %d, flat share %g, widest %g\n", same ? "same bits" : "DIFFERENT", n, k, share, widest);
		return same && share > 0.f && widest > 0.f ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
