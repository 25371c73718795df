// Call sites of the clustering operators and the clustered source swap in the C++ shim (include/goicp_mi355.hpp), compiled like
// tests/shim_stat_outlier.cpp: syntax-only by tests/test_cluster_host.py, and as a program with -DSHIM_CLUSTER_MAIN by
// tests/test_gpu_cluster.py, which runs it on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
using vec3 = Vec3;

// a tracking loop over raw scans: one model, one engine, of every scan only its largest clusters are registered
float track_clustered(std::vector<vec3>& model, std::vector<std::vector<vec3>>& scans, const goicp_source_pipeline* p, const goicp_cluster_select& s,
                      std::mutex& mtx, const goicp_params* params, size_t* kept)
{
	icp::FastGoICP engine(model, scans[0], 1e-3f, mtx, params);
	float last = -1.f;
	for (size_t i = 1; i < scans.size(); i++) {
		*kept = engine.set_source(scans[i], p, s);     // finished is false again, the poses are the identity
		if (engine.finished || *kept == 0 || *kept > scans[i].size()) return -1.f;
		engine.run();
		last = engine.get_best_error();
	}
	return last;
}

// the operator level: the registration lends its device
size_t largest_cluster(const icp::Registration& reg, const std::vector<vec3>& scan, float radius, int min_neighbors, std::vector<vec3>& kept,
                       std::vector<int32_t>& label, std::vector<int32_t>& sizes)
{
	reg.cluster(scan, scan.size(), radius, min_neighbors, label, &sizes);
	goicp_cluster_select s;
	goicp_cluster_select_default(&s);
	s.radius = radius; s.min_neighbors = min_neighbors; s.max_clusters = 1;
	return reg.cluster_filter(scan, scan.size(), s, kept);
}

#ifdef SHIM_CLUSTER_MAIN
// argv: model.f32 data.f32 radius min_neighbors -- every 10th data point plus a copy of every 100th moved beside the cloud (a second
// object); the device operators against the host functions, then the clustered swap against a fresh engine on the host function's output
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
	if (argc < 5) return 2;
	try {
		goicp_cluster_select s;
		goicp_cluster_select_default(&s);
		if (s.radius != 0.f || s.min_neighbors != 0 || s.min_size != 0 || s.max_clusters != 0 || sizeof(s) != 16) return 2;
		s.radius = (float)std::atof(argv[3]);
		s.min_neighbors = std::atoi(argv[4]);
		s.max_clusters = 1;
		std::vector<vec3> model = read_f32(argv[1], 1), scan = read_f32(argv[2], 10), extra = read_f32(argv[2], 100);
		if (model.empty() || scan.empty() || extra.empty()) return 2;
		for (const vec3& q : extra) scan.push_back(vec3(q[0] * 0.1f + 3.f, q[1] * 0.1f, q[2] * 0.1f));
		std::vector<std::vector<vec3>> scans{read_f32(argv[2], 60), scan};
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 64;
		const size_t n = scan.size();
		// the host functions
		std::vector<int32_t> hlabel(n), hsizes(n);
		size_t hc = 0, hm = 0;
		check(goicp_cluster_host(reinterpret_cast<const float*>(scan.data()), n, s.radius, s.min_neighbors, hlabel.data(), hsizes.data(), &hc));
		hsizes.resize(hc);
		std::vector<vec3> hkept(n);
		check(goicp_cluster_filter_host(reinterpret_cast<const float*>(scan.data()), n, &s, reinterpret_cast<float*>(hkept.data()), nullptr, nullptr, &hm));
		hkept.resize(hm);
		if (hc < 2 || hm == 0 || hm >= n) return 2;        // the case must have a second cluster to drop
		// the device operators
		icp::Registration reg(model, model.size(), scans[0], scans[0].size(), 1e-3f, &params);
		std::vector<int32_t> label, sizes;
		std::vector<vec3> kept;
		const size_t m = largest_cluster(reg, scan, s.radius, s.min_neighbors, kept, label, sizes);
		const bool ops = label == hlabel && sizes == hsizes && m == hm && std::memcmp(kept.data(), hkept.data(), sizeof(vec3) * hm) == 0;
		// the swap
		std::mutex mtx, mtx2;
		size_t swapped_kept = 0;
		const float swapped = track_clustered(model, scans, nullptr, s, mtx, &params, &swapped_kept);
		icp::FastGoICP fresh(model, hkept, 1e-3f, mtx2, &params);
		fresh.run();
		const float ref = fresh.get_best_error();
		unsigned a, b;
		std::memcpy(&a, &swapped, 4); std::memcpy(&b, &ref, 4);
		std::printf("swapped %08x fresh %08x kept %zu host %zu of %zu, %zu clusters, operators %s\n", a, b, swapped_kept, hm, n, hc, ops ? "agree" : "DIFFER");
		return a == b && swapped_kept == hm && ops ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
