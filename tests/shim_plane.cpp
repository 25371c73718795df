// Call sites of the plane segmentation and the segmented source swap in the C++ shim (include/goicp_mi355.hpp), compiled like
// tests/shim_cluster.cpp: syntax-only by tests/test_plane_host.py, and as a program with -DSHIM_PLANE_MAIN by tests/test_gpu_plane.py,
// which runs it on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
using vec3 = Vec3;

// a tracking loop over raw tabletop scans: one model, one engine; of every scan the table goes, then only the largest cluster is registered
float track_segmented(std::vector<vec3>& model, std::vector<std::vector<vec3>>& scans, const goicp_source_pipeline* p, const goicp_plane_select& pl,
                      const goicp_cluster_select* s, std::mutex& mtx, const goicp_params* params, size_t* kept)
{
	icp::FastGoICP engine(model, scans[0], 1e-3f, mtx, params);
	float last = -1.f;
	for (size_t i = 1; i < scans.size(); i++) {
		*kept = engine.set_source(scans[i], p, pl, s);
		if (engine.finished || *kept == 0 || *kept > scans[i].size()) return -1.f;
		engine.run();
		last = engine.get_best_error();
	}
	return last;
}

// the operator level: the registration lends its device
size_t without_floor(const icp::Registration& reg, const std::vector<vec3>& scan, float distance, std::vector<vec3>& kept, std::vector<int32_t>& label,
                     std::vector<goicp_plane>& planes)
{
	goicp_plane_select sel;
	goicp_plane_select_default(&sel);
	sel.distance = distance; sel.refine = 1; sel.seed = 7;
	reg.segment_plane(scan, scan.size(), sel, label, planes);
	std::vector<int32_t> index;
	return reg.plane_filter(scan, scan.size(), sel, kept, &index, &planes);
}

#ifdef SHIM_PLANE_MAIN
// argv: model.f32 data.f32 distance iterations -- every 10th data point on a floor of 60 % as many points at the cloud's min y (a fixed
// integer sequence gives its positions and its noise of +- distance / 2); the device operators against the host functions, then the
// segmented swap against a fresh engine on the host function's output
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
		goicp_plane_select sel;
		goicp_plane_select_default(&sel);
		if (sel.distance != 0.f || sel.iterations != 0 || sel.refine != 0 || sel.max_planes != 0 || sel.min_inliers != 0 || sel.seed != 0 || sizeof(sel) != 32 ||
		    sizeof(goicp_plane) != 40)
			return 2;
		sel.distance = (float)std::atof(argv[3]);
		sel.iterations = std::atoi(argv[4]);
		sel.refine = 1; sel.max_planes = 1; sel.seed = 7;
		std::vector<vec3> model = read_f32(argv[1], 1), object = read_f32(argv[2], 10);
		if (model.empty() || object.size() < 100) return 2;
		float lo[3] = {object[0][0], object[0][1], object[0][2]}, hi[3] = {lo[0], lo[1], lo[2]};
		for (const vec3& q : object)
			for (int k = 0; k < 3; k++) { lo[k] = q[k] < lo[k] ? q[k] : lo[k]; hi[k] = q[k] > hi[k] ? q[k] : hi[k]; }
		const size_t nf = object.size() * 6 / 10;
		unsigned long long state = 12345;
		auto unit = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (float)(state >> 40) / 16777216.f; };
		// object and floor interleaved, so neither is a prefix of the cloud
		std::vector<vec3> scan;
		for (size_t i = 0, j = 0; i < object.size() || j < nf;) {
			if (i < object.size()) scan.push_back(object[i++]);
			if (j < nf && (i * 6 >= j * 10 || i == object.size())) {
				const float x = lo[0] + (hi[0] - lo[0]) * unit(), z = lo[2] + (hi[2] - lo[2]) * unit();
				scan.push_back(vec3(x, lo[1] + sel.distance * (unit() - 0.5f), z));
				j++;
			}
		}
		std::vector<std::vector<vec3>> scans{read_f32(argv[2], 60), scan};
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 64;
		const size_t n = scan.size();
		// the host functions
		std::vector<int32_t> hlabel(n), hindex(n);
		std::vector<goicp_plane> hplanes(GOICP_PLANE_MAX_PLANES), hplanes2(GOICP_PLANE_MAX_PLANES);
		size_t hc = 0, hc2 = 0, hm = 0;
		check(goicp_segment_plane_host(reinterpret_cast<const float*>(scan.data()), n, &sel, hlabel.data(), hplanes.data(), &hc));
		hplanes.resize(hc);
		std::vector<vec3> hkept(n);
		check(goicp_plane_filter_host(reinterpret_cast<const float*>(scan.data()), n, &sel, reinterpret_cast<float*>(hkept.data()), hindex.data(), hplanes2.data(), &hc2,
		                              &hm));
		hkept.resize(hm);
		if (hc != 1 || hc2 != 1 || (size_t)hplanes[0].inliers < nf * 9 / 10 || hm == 0 || hm + (size_t)hplanes[0].inliers != n) return 2;   // the floor must go
		// the device operators
		icp::Registration reg(model, model.size(), scans[0], scans[0].size(), 1e-3f, &params);
		std::vector<int32_t> label;
		std::vector<goicp_plane> planes;
		std::vector<vec3> kept;
		sel.seed = 7;
		const size_t m = without_floor(reg, scan, sel.distance, kept, label, planes);      // 1000 hypotheses: its own defaults
		goicp_plane_select dflt = sel;
		dflt.iterations = 0;
		std::vector<int32_t> dlabel(n);
		std::vector<goicp_plane> dplanes(GOICP_PLANE_MAX_PLANES);
		std::vector<vec3> dkept(n);
		size_t dc = 0, dm = 0;
		check(goicp_segment_plane_host(reinterpret_cast<const float*>(scan.data()), n, &dflt, dlabel.data(), dplanes.data(), &dc));
		dplanes.resize(dc);
		check(goicp_plane_filter_host(reinterpret_cast<const float*>(scan.data()), n, &dflt, reinterpret_cast<float*>(dkept.data()), nullptr, nullptr, nullptr, &dm));
		bool ops = label == dlabel && planes.size() == dc && m == dm && std::memcmp(kept.data(), dkept.data(), sizeof(vec3) * dm) == 0;
		for (size_t q = 0; ops && q < dc; q++) ops = std::memcmp(&planes[q], &dplanes[q], sizeof(goicp_plane)) == 0;
		// the same with the caller's own selection
		std::vector<int32_t> label2, index2;
		std::vector<goicp_plane> planes2, planes3;
		std::vector<vec3> kept2;
		reg.segment_plane(scan, n, sel, label2, planes2);
		const size_t m2 = reg.plane_filter(scan, n, sel, kept2, &index2, &planes3);
		ops = ops && label2 == hlabel && planes2.size() == 1 && planes3.size() == 1 && std::memcmp(&planes2[0], &hplanes[0], sizeof(goicp_plane)) == 0 &&
		      std::memcmp(&planes3[0], &hplanes2[0], sizeof(goicp_plane)) == 0 && m2 == hm && std::memcmp(kept2.data(), hkept.data(), sizeof(vec3) * hm) == 0;
		hindex.resize(hm);
		ops = ops && index2 == hindex;
		// the swap
		std::mutex mtx, mtx2;
		size_t swapped_kept = 0;
		const float swapped = track_segmented(model, scans, nullptr, sel, nullptr, mtx, &params, &swapped_kept);
		icp::FastGoICP fresh(model, hkept, 1e-3f, mtx2, &params);
		fresh.run();
		const float ref = fresh.get_best_error();
		unsigned a, b;
		std::memcpy(&a, &swapped, 4); std::memcpy(&b, &ref, 4);
		std::printf("swapped %08x fresh %08x kept %zu host %zu of %zu, plane of %d inliers, operators %s\n", a, b, swapped_kept, hm, n, (int)hplanes[0].inliers,
		            ops ? "agree" : "DIFFER");
		return a == b && swapped_kept == hm && ops ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
