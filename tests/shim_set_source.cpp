// Call sites of the source swap in the C++ shim (include/goicp_mi355.hpp), compiled like tests/shim_callsites.cpp: syntax-only by
// tests/test_source_order_host.py (with the shim's own Mat3 / Vec3 and with glm types on the caller's side, -DSHIM_WITH_GLM), and as a
// program with -DSHIM_SET_SOURCE_MAIN by tests/test_gpu_set_source.py, which runs it on the GPU.
#ifdef SHIM_WITH_GLM
#include <glm/glm.hpp>
#endif
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
#ifdef SHIM_WITH_GLM
using vec3 = glm::vec3;
#else
using vec3 = Vec3;
#endif

// a tracking loop: one model, a stream of scans, one engine
float track(std::vector<vec3>& model, std::vector<std::vector<vec3>>& scans, std::mutex& mtx, const goicp_params* params)
{
	icp::FastGoICP engine(model, scans[0], 1e-3f, mtx, params);
	engine.run();
	float last = engine.get_best_error();
	for (size_t i = 1; i < scans.size(); i++) {
		engine.set_source(scans[i]);              // finished is false again, the poses are the identity
		if (engine.finished) return -1.f;
		engine.run();
		last = engine.get_best_error();
	}
	return last;
}

// the operator level: the registration alone
float rescore(icp::Registration& reg, const std::vector<vec3>& scan)
{
	reg.set_source(scan, scan.size());
	float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0}, sse = 0.f;
	check(goicp_eval_sse(reg.handle(), I, z, &sse));
	return sse;
}

#ifdef SHIM_SET_SOURCE_MAIN
// argv: model.f32 data.f32 -- registers every 60th data point, swaps to every 15th, and prints the swapped engine's error next to a
// fresh engine's on the same pair (the two must print the same bits)
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
	if (argc < 3) return 2;
	try {
		std::vector<vec3> model = read_f32(argv[1], 1);
		std::vector<std::vector<vec3>> scans{read_f32(argv[2], 60), read_f32(argv[2], 15)};
		if (model.empty() || scans[0].empty() || scans[1].empty()) return 2;
		goicp_params p;
		goicp_params_default(&p);
		p.dt_size = 64;
		std::mutex mtx;
		const float swapped = track(model, scans, mtx, &p);
		std::mutex mtx2;
		icp::FastGoICP fresh(model, scans[1], 1e-3f, mtx2, &p);
		fresh.run();
		const float ref = fresh.get_best_error();
		unsigned a, b;
		std::memcpy(&a, &swapped, 4); std::memcpy(&b, &ref, 4);
		std::printf("swapped %08x fresh %08x\n", a, b);
		icp::Registration reg(model, model.size(), scans[0], scans[0].size(), 1e-3f, &p);
		std::printf("rescore %g\n", rescore(reg, scans[1]));
		return a == b ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
