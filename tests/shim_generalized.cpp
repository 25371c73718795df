// Call sites of the generalized (plane-to-plane) ICP modifier in the C++ shim (include/goicp_mi355.hpp), compiled like tests/shim_symmetric.cpp:
// syntax-only by tests/test_icp_generalized_host.py, and as a program with -DSHIM_GENERALIZED_MAIN by tests/test_gpu_icp_generalized.py, which
// runs it on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
using vec3 = Vec3;

// metric 1 in its generalized form with the given epsilon, the source normals estimated from k neighbours; what the handle then reports
icp::Registration::IcpGeneralized enable_generalized(icp::Registration& reg, float epsilon, int k)
{
	reg.set_icp_options(1, 16);
	reg.set_icp_generalized(true, epsilon, k);
	return reg.get_icp_generalized();
}

// back to plain point-to-plane; the flag's epsilon and k stay stored
bool disable_generalized(icp::Registration& reg, float epsilon, int k)
{
	reg.set_icp_generalized(false, epsilon, k);
	return reg.get_icp_generalized().enabled;
}

#ifdef SHIM_GENERALIZED_MAIN
// argv: model.f32 data.f32 k -- an engine on every 10th data point: two generalized ICP runs (the same bits), a point-to-plane run between
// them (other bits), and the symmetric flag refused while this one is on
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
		const icp::Registration::IcpGeneralized s = enable_generalized(reg, 0.01f, k);
		const Run a = run(reg);
		bool refused = false;
		try { reg.set_icp_symmetric(true, k); } catch (const std::exception&) { refused = true; }
		const bool off = !disable_generalized(reg, 0.01f, k);
		const Run plane = run(reg);
		enable_generalized(reg, 0.01f, k);
		const Run b = run(reg);
		const bool same_runs = std::memcmp(&a, &b, sizeof(Run)) == 0, other = std::memcmp(&a, &plane, sizeof(Run)) != 0;
		std::printf("%s: %zu points, k %d, epsilon %g, enabled %d, %d iterations, err %g\n", same_runs ? "same bits" : "DIFFERENT", data.size(),
		            s.source_normal_k, s.epsilon, (int)s.enabled, (int)a.iters, a.err);
		return same_runs && other && refused && off && s.enabled && s.epsilon == 0.01f && s.source_normal_k == k && !s.user_normals && a.iters > 1 ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
