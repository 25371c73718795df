// Call sites of the symmetric point-to-plane modifier in the C++ shim (include/goicp_mi355.hpp), compiled like tests/shim_normals.cpp:
// syntax-only by tests/test_icp_symmetric_host.py, and as a program with -DSHIM_SYMMETRIC_MAIN by tests/test_gpu_icp_symmetric.py, which runs
// it on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
using vec3 = Vec3;

// metric 1 in its symmetric form, the source normals estimated from k neighbours; what the handle then reports
icp::Registration::IcpSymmetric enable_symmetric(icp::Registration& reg, int k, std::vector<vec3>& normals)
{
	reg.set_icp_options(1, 16);
	reg.set_icp_symmetric(true, k);
	reg.source_normals(normals);
	return reg.icp_symmetric();
}

// a sensor's own normals in the place of the estimated ones
bool use_sensor_normals(icp::Registration& reg, const std::vector<vec3>& normals)
{
	reg.set_source_normals(normals);
	return reg.icp_symmetric().user_normals;
}

#ifdef SHIM_SYMMETRIC_MAIN
// argv: model.f32 data.f32 k -- an engine on every 10th data point: the source normals against the host function (the same bits), two
// symmetric ICP runs (the same bits), and the same run again on the handle's own normals handed back in as the caller's
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

struct Run { float R[9], t[3], err; int32_t iters; };
static Run run(icp::Registration& reg)
{
	Run r{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0.01f, -0.02f, 0.005f}, 0.f, 0};
	check(goicp_icp_run(reg.handle(), r.R, r.t, 200, 1e-7f, &r.err, &r.iters));
	return r;
}

int main(int argc, char** argv)
{
	if (argc < 4) return 2;
	try {
		const int k = std::atoi(argv[3]);
		std::vector<vec3> model = read_f32(argv[1], 1), data = read_f32(argv[2], 10);
		if (model.empty() || data.size() < 64) return 2;
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 64;
		icp::Registration reg(model, model.size(), data, data.size(), 1e-3f, &params);
		std::vector<vec3> normals;
		const icp::Registration::IcpSymmetric s = enable_symmetric(reg, k, normals);
		const size_t n = data.size();
		std::vector<float> host_n(3 * n);
		check(goicp_estimate_normals_host(reinterpret_cast<const float*>(data.data()), n, k, nullptr, host_n.data(), nullptr, nullptr));
		const bool same_normals = normals.size() == n && std::memcmp(host_n.data(), normals.data(), sizeof(float) * 3 * n) == 0;
		const Run a = run(reg), b = run(reg);
		const bool user = use_sensor_normals(reg, normals);
		const Run c = run(reg);
		const bool same_runs = std::memcmp(&a, &b, sizeof(Run)) == 0 && std::memcmp(&a, &c, sizeof(Run)) == 0;
		std::printf("%s: %zu points, k %d, enabled %d, user %d, %d iterations, err %g\n", same_normals && same_runs ? "same bits" : "DIFFERENT", n,
		            s.source_normal_k, (int)s.enabled, (int)user, (int)a.iters, a.err);
		return same_normals && same_runs && s.enabled && s.source_normal_k == k && !s.user_normals && user && a.iters > 1 ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
