// Call sites of the RANSAC pose estimation in the C++ shim (include/goicp_mi355.hpp), compiled like tests/shim_plane.cpp: syntax-only by
// tests/test_ransac_host.py, and as a program with -DSHIM_RANSAC_MAIN by tests/test_gpu_ransac.py, which runs it on the GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "goicp_mi355.hpp"

using namespace goicp_mi355;
using vec3 = Vec3;

// the operator level: the registration lends its device.  From the matcher's output to start poses for icp_run_batch
size_t start_poses(const icp::Registration& reg, const std::vector<vec3>& src, const std::vector<vec3>& tgt, const std::vector<int32_t>& index,
                   const std::vector<float>& d2, const std::vector<float>& d2_second, const std::vector<uint8_t>& mutual, float distance,
                   std::vector<goicp_ransac_pose_result>& poses, std::vector<int32_t>& corr, std::vector<uint8_t>& inlier)
{
	if (icp::Registration::select_matches(index, d2, d2_second, &mutual, 0.9f, true, corr) < 3) return 0;
	goicp_ransac_pose_select sel;
	goicp_ransac_pose_select_default(&sel);
	sel.distance = distance; sel.iterations = 1000; sel.max_poses = 4; sel.seed = 7;
	return reg.ransac_pose(src, tgt, corr, sel, poses, &inlier);
}

#ifdef SHIM_RANSAC_MAIN
// argv: model.f32 data.f32 -- every 40th data point and its image under a fixed pose as the target, every second correspondence true and
// the others shifted by a fixed integer sequence; the device operator through the shim against the host function, as bytes
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
		goicp_ransac_pose_select sel;
		goicp_ransac_pose_select_default(&sel);
		if (sel.distance != 0.f || sel.iterations != 0 || sel.refine != 1 || sel.max_poses != 0 || sel.min_inliers != 0 || sel.seed != 0 || sizeof(sel) != 32 ||
		    sizeof(goicp_ransac_pose_result) != 60)
			return 2;
		std::vector<vec3> model = read_f32(argv[1], 1), src = read_f32(argv[2], 40);
		if (model.empty() || src.size() < 100) return 2;
		const size_t n = src.size();
		// a quarter turn about z and a shift; the matcher's output is made up: index i for every second query, (i * 7 + 3) % n for the others
		std::vector<vec3> tgt(n);
		for (size_t i = 0; i < n; i++) tgt[i] = vec3(-src[i][1] + 0.1f, src[i][0] - 0.2f, src[i][2] + 0.05f);
		std::vector<int32_t> index(n), corr;
		std::vector<float> d2(n), second(n);
		std::vector<uint8_t> mutual(n), inlier;
		for (size_t i = 0; i < n; i++) {
			index[i] = (int32_t)(i % 2 == 0 ? i : (i * 7 + 3) % n);
			d2[i] = 1.f; second[i] = i % 5 == 4 ? 1.1f : 2.f;      // every fifth fails the ratio test at 0.9: 1 > 0.81 * 1.1
			mutual[i] = i % 3 != 2;
		}
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 64;
		std::vector<vec3> small = read_f32(argv[2], 60);
		icp::Registration reg(model, model.size(), small, small.size(), 1e-3f, &params);
		std::vector<goicp_ransac_pose_result> poses;
		const size_t c = start_poses(reg, src, tgt, index, d2, second, mutual, 0.01f, poses, corr, inlier);
		// the host functions
		sel.distance = 0.01f; sel.iterations = 1000; sel.max_poses = 4; sel.seed = 7;
		size_t kept = 0;
		for (size_t i = 0; i < n; i++) kept += mutual[i] && i % 5 != 4;
		std::vector<goicp_ransac_pose_result> hposes(GOICP_RANSAC_POSE_MAX_POSES);
		std::vector<uint8_t> hinlier(corr.size() / 2);
		size_t hc = 0;
		check(goicp_ransac_pose_host(reinterpret_cast<const float*>(src.data()), n, reinterpret_cast<const float*>(tgt.data()), n, corr.data(), corr.size() / 2, &sel,
		                             hposes.data(), &hc, hinlier.data()));
		bool ops = corr.size() == 2 * kept && c == hc && c >= 1 && inlier == hinlier;
		for (size_t q = 0; ops && q < hc; q++) ops = std::memcmp(&poses[q], &hposes[q], sizeof(goicp_ransac_pose_result)) == 0;
		const bool found = c >= 1 && std::fabs(poses[0].R[1] + 1.f) < 1e-4f && std::fabs(poses[0].R[3] - 1.f) < 1e-4f && std::fabs(poses[0].t[0] - 0.1f) < 1e-3f &&
		                   std::fabs(poses[0].t[1] + 0.2f) < 1e-3f && std::fabs(poses[0].t[2] - 0.05f) < 1e-3f;
		std::printf("%zu correspondences of %zu queries, %zu poses, pose 0 with %d inliers %s, operators %s\n", corr.size() / 2, n, c, c ? (int)poses[0].inliers : 0,
		            found ? "is the pose" : "IS NOT THE POSE", ops ? "agree" : "DIFFER");
		return ops && found ? 0 : 1;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
}
#endif
