// Call sites of the filtered source swap in the C++ shim (include/goicp_mi355.hpp), compiled like tests/shim_voxel.cpp: syntax-only by
// tests/test_outlier_removal_host.py (with the shim's own Mat3 / Vec3 and with glm types on the caller's side, -DSHIM_WITH_GLM), and as a
// program with -DSHIM_OUTLIER_MAIN by tests/test_gpu_outlier_removal.py, which runs it on the GPU.
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

// a tracking loop over raw scans: one model, one engine, every scan reduced and cleaned on the device before it is registered
float track_filtered(std::vector<vec3>& model, std::vector<std::vector<vec3>>& scans, const goicp_source_filter& f, std::mutex& mtx,
                     const goicp_params* params, size_t* kept)
{
	icp::FastGoICP engine(model, scans[0], 1e-3f, mtx, params);
	float last = -1.f;
	for (size_t i = 1; i < scans.size(); i++) {
		*kept = engine.set_source(scans[i], f);       // finished is false again, the poses are the identity
		if (engine.finished || *kept == 0 || *kept > scans[i].size()) return -1.f;
		engine.run();
		last = engine.get_best_error();
	}
	return last;
}

// the operator level: the registration alone
float rescore_filtered(icp::Registration& reg, const std::vector<vec3>& scan, const goicp_source_filter& f, size_t* kept)
{
	*kept = reg.set_source(scan, scan.size(), f);
	float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0}, sse = 0.f;
	check(goicp_eval_sse(reg.handle(), I, z, &sse));
	return sse;
}

#ifdef SHIM_OUTLIER_MAIN
// argv: model.f32 data.f32 voxel radius min_neighbors -- creates an engine on every 60th data point, swaps to every 3rd behind the filter
// chain and registers; prints the error next to a fresh engine's on the host functions' output of the same cloud (the same bits)
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
	if (argc < 6) return 2;
	try {
		goicp_source_filter f;
		goicp_source_filter_default(&f);
		if (f.voxel != 0.f || f.radius != 0.f || f.min_neighbors != 0) return 2;
		f.voxel = (float)std::atof(argv[3]);
		f.radius = (float)std::atof(argv[4]);
		f.min_neighbors = std::atoi(argv[5]);
		std::vector<vec3> model = read_f32(argv[1], 1);
		std::vector<std::vector<vec3>> scans{read_f32(argv[2], 60), read_f32(argv[2], 3)};
		if (model.empty() || scans[0].empty() || scans[1].empty()) return 2;
		goicp_params p;
		goicp_params_default(&p);
		p.dt_size = 64;
		std::mutex mtx;
		size_t kept = 0, m1 = 0, m = 0, kept2 = 0;
		const float swapped = track_filtered(model, scans, f, mtx, &p, &kept);
		std::vector<vec3> reduced(scans[1].size());
		check(goicp_voxel_downsample_host(reinterpret_cast<const float*>(scans[1].data()), scans[1].size(), f.voxel,
		                                  reinterpret_cast<float*>(reduced.data()), nullptr, &m1));
		reduced.resize(m1);
		std::vector<vec3> cleaned(m1);
		check(goicp_radius_outlier_removal_host(reinterpret_cast<const float*>(reduced.data()), m1, f.radius, f.min_neighbors,
		                                        reinterpret_cast<float*>(cleaned.data()), nullptr, nullptr, &m));
		cleaned.resize(m);
		if (m == 0 || m >= m1) return 2;              // the case must drop something and keep something
		std::mutex mtx2;
		icp::FastGoICP fresh(model, cleaned, 1e-3f, mtx2, &p);
		fresh.run();
		const float ref = fresh.get_best_error();
		unsigned a, b;
		std::memcpy(&a, &swapped, 4); std::memcpy(&b, &ref, 4);
		std::printf("swapped %08x fresh %08x kept %zu host %zu of %zu\n", a, b, kept, m, m1);
		icp::Registration reg(model, model.size(), scans[0], scans[0].size(), 1e-3f, &p);
		std::printf("rescore %g\n", rescore_filtered(reg, scans[1], f, &kept2));
		return a == b && kept == m && kept2 == m ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
