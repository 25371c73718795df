// Call sites of the voxel-grid source swap in the C++ shim (include/goicp_mi355.hpp), compiled like tests/shim_set_source.cpp: syntax-only
// by tests/test_voxel_downsample_host.py (with the shim's own Mat3 / Vec3 and with glm types on the caller's side, -DSHIM_WITH_GLM), and
// as a program with -DSHIM_VOXEL_MAIN by tests/test_gpu_voxel_downsample.py, which runs it on the GPU.
#ifdef SHIM_WITH_GLM
#include <glm/glm.hpp>
#endif
#include <cstdio>
#include <cstdlib>
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

// a tracking loop over raw scans: one model, one engine, every scan reduced on the device before it is registered
float track_voxel(std::vector<vec3>& model, std::vector<std::vector<vec3>>& scans, float voxel, std::mutex& mtx, const goicp_params* params, size_t* kept)
{
	icp::FastGoICP engine(model, scans[0], 1e-3f, mtx, params);
	float last = -1.f;
	for (size_t i = 1; i < scans.size(); i++) {
		*kept = engine.set_source(scans[i], voxel);   // finished is false again, the poses are the identity
		if (engine.finished || *kept == 0 || *kept > scans[i].size()) return -1.f;
		engine.run();
		last = engine.get_best_error();
	}
	return last;
}

// the operator level: the registration alone
float rescore_voxel(icp::Registration& reg, const std::vector<vec3>& scan, float voxel, size_t* kept)
{
	*kept = reg.set_source(scan, scan.size(), voxel);
	float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0}, sse = 0.f;
	check(goicp_eval_sse(reg.handle(), I, z, &sse));
	return sse;
}

#ifdef SHIM_VOXEL_MAIN
// argv: model.f32 data.f32 voxel -- creates an engine on every 60th data point, swaps to every 3rd behind the voxel grid and registers;
// prints the error next to a fresh engine's on the host function's output of the same cloud (the two must print the same bits)
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
		const float voxel = (float)std::atof(argv[3]);
		std::vector<vec3> model = read_f32(argv[1], 1);
		std::vector<std::vector<vec3>> scans{read_f32(argv[2], 60), read_f32(argv[2], 3)};
		if (model.empty() || scans[0].empty() || scans[1].empty()) return 2;
		goicp_params p;
		goicp_params_default(&p);
		p.dt_size = 64;
		std::mutex mtx;
		size_t kept = 0, m = 0, kept2 = 0;
		const float swapped = track_voxel(model, scans, voxel, mtx, &p, &kept);
		std::vector<vec3> reduced(scans[1].size());
		check(goicp_voxel_downsample_host(reinterpret_cast<const float*>(scans[1].data()), scans[1].size(), voxel,
		                                  reinterpret_cast<float*>(reduced.data()), nullptr, &m));
		reduced.resize(m);
		std::mutex mtx2;
		icp::FastGoICP fresh(model, reduced, 1e-3f, mtx2, &p);
		fresh.run();
		const float ref = fresh.get_best_error();
		unsigned a, b;
		std::memcpy(&a, &swapped, 4); std::memcpy(&b, &ref, 4);
		std::printf("swapped %08x fresh %08x kept %zu host %zu\n", a, b, kept, m);
		icp::Registration reg(model, model.size(), scans[0], scans[0].size(), 1e-3f, &p);
		std::printf("rescore %g\n", rescore_voxel(reg, scans[1], voxel, &kept2));
		return a == b && kept == m && kept2 == m ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
