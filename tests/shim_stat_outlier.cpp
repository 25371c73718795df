// Call sites of the three-stage source swap in the C++ shim (include/goicp_mi355.hpp), compiled like tests/shim_outlier.cpp: syntax-only by
// tests/test_stat_outlier_host.py, and as a program with -DSHIM_STAT_MAIN by tests/test_gpu_stat_outlier.py, which runs it on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
using vec3 = Vec3;

// a tracking loop over raw scans: one model, one engine, every scan reduced and cleaned on the device before it is registered
float track_pipeline(std::vector<vec3>& model, std::vector<std::vector<vec3>>& scans, const goicp_source_pipeline& p, std::mutex& mtx,
                     const goicp_params* params, size_t* kept)
{
	icp::FastGoICP engine(model, scans[0], 1e-3f, mtx, params);
	float last = -1.f;
	for (size_t i = 1; i < scans.size(); i++) {
		*kept = engine.set_source(scans[i], p);       // finished is false again, the poses are the identity
		if (engine.finished || *kept == 0 || *kept > scans[i].size()) return -1.f;
		engine.run();
		last = engine.get_best_error();
	}
	return last;
}

// the operator level: the registration alone
float rescore_pipeline(icp::Registration& reg, const std::vector<vec3>& scan, const goicp_source_pipeline& p, size_t* kept)
{
	*kept = reg.set_source(scan, scan.size(), p);
	float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0}, sse = 0.f;
	check(goicp_eval_sse(reg.handle(), I, z, &sse));
	return sse;
}

#ifdef SHIM_STAT_MAIN
// argv: model.f32 data.f32 voxel neighbors std_ratio -- creates an engine on every 60th data point, swaps to every 3rd behind the chain and
// registers; prints the error next to a fresh engine's on the host functions' output of the same cloud (the same bits)
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
		goicp_source_pipeline p;
		goicp_source_pipeline_default(&p);
		if (p.voxel != 0.f || p.stat_neighbors != 0 || p.stat_std_ratio != 0.f || p.radius != 0.f || p.min_neighbors != 0) return 2;
		p.voxel = (float)std::atof(argv[3]);
		p.stat_neighbors = std::atoi(argv[4]);
		p.stat_std_ratio = (float)std::atof(argv[5]);
		std::vector<vec3> model = read_f32(argv[1], 1);
		std::vector<std::vector<vec3>> scans{read_f32(argv[2], 60), read_f32(argv[2], 3)};
		if (model.empty() || scans[0].empty() || scans[1].empty()) return 2;
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 64;
		std::mutex mtx;
		size_t kept = 0, m1 = 0, m = 0, kept2 = 0;
		const float swapped = track_pipeline(model, scans, p, mtx, &params, &kept);
		std::vector<vec3> reduced(scans[1].size());
		check(goicp_voxel_downsample_host(reinterpret_cast<const float*>(scans[1].data()), scans[1].size(), p.voxel,
		                                  reinterpret_cast<float*>(reduced.data()), nullptr, &m1));
		reduced.resize(m1);
		std::vector<vec3> cleaned(m1);
		check(goicp_statistical_outlier_removal_host(reinterpret_cast<const float*>(reduced.data()), m1, p.stat_neighbors, p.stat_std_ratio,
		                                             reinterpret_cast<float*>(cleaned.data()), nullptr, nullptr, nullptr, &m));
		cleaned.resize(m);
		if (m == 0 || m >= m1) return 2;              // the case must drop something and keep something
		std::mutex mtx2;
		icp::FastGoICP fresh(model, cleaned, 1e-3f, mtx2, &params);
		fresh.run();
		const float ref = fresh.get_best_error();
		unsigned a, b;
		std::memcpy(&a, &swapped, 4); std::memcpy(&b, &ref, 4);
		std::printf("swapped %08x fresh %08x kept %zu host %zu of %zu\n", a, b, kept, m, m1);
		icp::Registration reg(model, model.size(), scans[0], scans[0].size(), 1e-3f, &params);
		std::printf("rescore %g\n", rescore_pipeline(reg, scans[1], p, &kept2));
		return a == b && kept == m && kept2 == m ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
