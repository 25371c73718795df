// goicp_cli: headless replacement for the reference's viewer main (src/main.cpp:14-187).  Takes the
// reference's .toml unchanged:  goicp_cli <config.toml> [--iters N] [--trim-fraction F] [--verbose] [--seed S] [--ranks N] [--reference-root]
//                                [--point-to-plane] [--normal-k K] [--symmetric [--source-normal-k K]] [--generalized [--gicp-epsilon E]] [--max-corr-dist D] [--robust-kernel {huber,cauchy,gm,tukey} --robust-scale C]
//                                [--trunc-dist D] [--information [--information-rank-tol X]] [--source-list FILE] [--voxel V] [--target-voxel V]
//                                [--outlier-radius R --outlier-min-neighbors K] [--target-outlier-radius R --target-outlier-min-neighbors K]
//                                [--stat-neighbors K --stat-std-ratio A] [--target-stat-neighbors K --target-stat-std-ratio A]
//                                [--plane-distance D [--plane-iterations T] [--plane-max P] [--plane-min-inliers S] [--plane-seed X] [--plane-no-refine]]
//   --ranks N   (modes 3/4) shard the rotation-cube search over N GPUs of this node: N engines (device r for rank r),
//               N host threads, RCCL all-reduce / broadcast over xGMI (goicp_register_multi_gpu)
//   --reference-root   search the reference CPU path's roots ([-pi,pi]^3 x [-0.5,0.5]^3, src/goicp/jly_goicp.cpp:44-53) and
//               ignore the TOML's [params.rotation] / [params.translation] / search_depth -- which the reference declares
//               (src/common.h:157-169) but never applies.  WITHOUT this flag the ranges ARE applied (the configs ship
//               translation +-1.0: a root of width 2, 8x the volume of the CPU path's), so node counts and times on the
//               reference's own .toml files are then not comparable with the strict-order goldens: use the flag for parity runs.
//   --point-to-plane   every ICP of the run is point-to-plane (goicp_set_icp_options metric 1; --normal-k K neighbours per target
//               normal, default 16).  Refused together with --ranks N > 1: the multi-GPU registration runs point-to-point ICP
//   --symmetric   implies --point-to-plane; every ICP of the run takes the symmetric point-to-plane form over the normals of both clouds
//               (goicp_set_icp_symmetric; --source-normal-k K neighbours per source normal, 3..32, default 16).  Refused together with
//               --ranks N > 1 and --trim-fraction F > 0, and with K out of range -- before any device is touched
//   --generalized   implies --point-to-plane; every ICP of the run takes the generalized (plane-to-plane) form, each correspondence weighted by the
//               combined covariance of both clouds' normals (goicp_set_icp_generalized; --gicp-epsilon E in [1e-4, 1], default 1e-3;
//               --source-normal-k K as under --symmetric).  Refused together with --symmetric, --ranks N > 1 and --trim-fraction F > 0, and with
//               E out of range -- before any device is touched
//   --max-corr-dist D   every ICP of the run uses only correspondences within distance D (goicp_set_icp_gate; cloud units after
//               `resize`); output.toml then gets an [icp_gate] table with D and the inlier count of the final pose.  D must be a finite
//               number > 0, and the flag is refused together with --ranks N > 1 and --trim-fraction F > 0 -- before any device is touched
//   --robust-kernel {huber,cauchy,gm,tukey} --robust-scale C   every ICP of the run weights its correspondences by that M-estimator with
//               scale C (goicp_set_icp_robust; cloud units after `resize`).  C must be a finite number > 0, both flags are needed, and they are
//               refused together with --ranks N > 1, --trim-fraction F > 0 and --max-corr-dist -- before any device is touched
//   --trunc-dist D   the SEARCH minimises the truncated cost sum min(DT(R p + t), D)^2 instead of the plain sum of squares
//               (goicp_set_search_truncation; cloud units after `resize`): bounds, pose scores and the reported best error are all truncated,
//               and output.toml gets a [search] table with trunc_dist.  Goes with --max-corr-dist, --point-to-plane and --robust-kernel (they
//               only change the refinement).  D must be a finite number > 0, and the flag is refused together with --ranks N > 1 and
//               --trim-fraction F > 0 -- before any device is touched
//   --information   after the run, the information matrix and covariance of the final pose (goicp_pose_information: the handle's metric and
//               weights, pivot = the transformed source centroid): one line with rank and sigma, and output.toml gets an [information] table
//               (rank, sigma2, inliers, weight_sum, eigenvalues, information and covariance as arrays of rows).  --information-rank-tol X sets
//               rank_tol (in [0, 1)).  Refused together with --ranks N > 1 -- before any device is touched
//   --source-list FILE   a stream of scans against one model: FILE names one cloud per line (blank lines and lines starting with # are
//               skipped; relative paths are tried as given, then beside FILE).  After the config's own source, each listed cloud is loaded
//               with the config's subsample, resize and the seed, swapped into the SAME engine (goicp_set_source: the target's distance
//               transform, k-d hierarchy and every option set above are kept) and registered; one line per cloud with the swap's
//               milliseconds, and io.output / io.visualization are written with .1, .2, ... before the extension.  Refused together with
//               --ranks N > 1 and when FILE cannot be read or names no cloud -- before any device is touched
//   --voxel V   the source -- and every cloud of --source-list -- is reduced to one centroid per occupied cell of a grid of pitch V (cloud
//               units after `resize`) before it is registered.  The config's own source is reduced on the host (goicp_voxel_downsample_host:
//               no engine exists yet), every listed cloud on the device as part of its swap (goicp_set_source_voxel: the same bits).
//               --target-voxel V reduces the target the same way, on the host, before the engine is created.  V must be a finite number > 0
//               -- refused before any device is touched; the .toml surface is the reference's and stays as it is
//   --outlier-radius R --outlier-min-neighbors K   (both or neither) radius outlier removal, after --voxel: a point of the source -- and
//               of every cloud of --source-list -- with fewer than K other points within R (cloud units after `resize`) is dropped before
//               the cloud is registered.  The config's own source is filtered on the host (goicp_radius_outlier_removal_host), every listed
//               cloud on the device as part of its swap (goicp_set_source_filtered: the same bits); each prints "kept m of n".
//               --target-outlier-radius R --target-outlier-min-neighbors K filter the target the same way, on the host, after
//               --target-voxel and before the engine is created.  R must be finite, > 0 and R * R a normal float, K an integer >= 1 --
//               refused before any device is touched
//   --stat-neighbors K --stat-std-ratio A   (both or neither) statistical outlier removal, after --voxel and before --outlier-radius: a
//               point of the source -- and of every cloud of --source-list -- whose mean distance to its K nearest neighbours lies more than
//               A sample deviations above the cloud's mean of it is dropped.  The config's own source is filtered on the host
//               (goicp_statistical_outlier_removal_host), every listed cloud on the device as part of its swap (goicp_set_source_pipeline:
//               the same bits); each prints "kept m of n".  --target-stat-neighbors K --target-stat-std-ratio A filter the target the same
//               way, on the host.  K must be an integer in 1..64, A a finite number >= 0 -- refused before any device is touched
//   --cluster-radius R [--cluster-min-neighbors K] [--cluster-min-size S] [--cluster-keep C]   Euclidean / DBSCAN clustering, after the other
//               filters: the points of the source -- and of every cloud of --source-list -- are grouped into the connected components of
//               the core points under distance R (a point is core with at least K other points within R; K = 0, the default, makes every
//               point core), and only the C largest clusters (default 1; 0 = all) with at least S members (default 0) stay.  The config's
//               own source is filtered on the host (goicp_cluster_filter_host), every listed cloud on the device as part of its swap
//               (goicp_set_source_clustered: the same bits); each prints "kept m of n".  The --target-cluster-* forms filter the target the
//               same way, on the host, before the engine is created.  R must be finite, > 0 and R * R a normal float, K, S and C integers
//               >= 0, and the three need --cluster-radius -- refused before any device is touched
//   --plane-distance D [--plane-iterations T] [--plane-max P] [--plane-min-inliers S] [--plane-seed X] [--plane-no-refine]   RANSAC plane removal,
//               after the neighbourhood filters and before --cluster-*: the points of the source -- and of every cloud of --source-list --
//               within D (cloud units after `resize`) of the dominant plane are dropped: the best of T three-point hypotheses (default 1000),
//               refit once by least squares over its inliers unless --plane-no-refine, for up to P planes in turn (default 1), each with at
//               least S inliers (default 0); X seeds the draws (default 0).  The config's own source is filtered on the host
//               (goicp_plane_filter_host), every listed cloud on the device as part of its swap (goicp_set_source_segmented: the same bits);
//               each prints "kept m of n".  The --target-plane-* forms filter the target the same way, on the host, before the engine is
//               created.  D must be a finite number > 0, T an integer in 0..65536, P in 0..8, S an integer >= 0, and the others need
//               --plane-distance -- refused before any device is touched
//   --estimate-normals IN OUT.ply [--normal-k K] [--viewpoint X,Y,Z]   a mode of its own that takes no config and registers nothing: per-point
//               normals and surface variation of the cloud IN from its K-point neighbourhoods (K counts the point itself, 3..32, default 16;
//               goicp_estimate_normals on the device when there is one, goicp_estimate_normals_host otherwise: the same bits), flipped
//               towards the viewpoint when one is given.  OUT.ply is an ASCII PLY with x y z nx ny nz curvature.  Refused together with
//               --ranks -- before any device is touched
//   --fpfh-match SRC TGT OUT.txt [--fpfh-k K] [--normal-k K] [--voxel V]   a mode of its own that takes no config and registers nothing: both
//               clouds, reduced by a voxel grid of pitch V on the host when --voxel is given, get normals from their K-point neighbourhoods
//               (--normal-k, 3..32, default 16, no viewpoint) and 33-bin FPFH descriptors over their K nearest other points (--fpfh-k, 1..32,
//               default 16); every descriptor of SRC is matched to its nearest of TGT (goicp_estimate_normals, goicp_fpfh and
//               goicp_match_features on the device when there is one, the _host forms otherwise: the same bits).  OUT.txt gets one line
//               `i j d2 d2_second` per mutual match.  Refused together with --ranks -- before any device is touched
//   --feature-init [--feature-voxel V] [--fpfh-k K] [--normal-k K] [--match-ratio R] [--ransac-distance D] [--ransac-iterations T]
//               [--ransac-poses K] [--ransac-seed X]   modes 0..2: the ICP starts from the best feature pose, not from the identity.  Both
//               clouds (reduced by a voxel grid of pitch V when given) get normals (--normal-k, 3..32, default 16) and FPFH descriptors
//               (--fpfh-k, 1..32, default 16) on the device; the mutual matches that pass the ratio test (--match-ratio, default 0 = none) go to
//               goicp_ransac_pose (inlier distance D, default 1.5 V; T hypotheses, default 100 000; K poses, default 1; seed X) and
//               goicp_icp_run refines the best-supported pose for --iters iterations.  With this flag alone --normal-k is the features' k; it
//               reaches the ICP options only together with --point-to-plane, --symmetric or --generalized.  Refused together with --ranks,
//               --source-list, modes 3/4 and a config with [io] output or visualization (those files report the engine's own state) --
//               before any device is touched
//   modes 0/1/2 (plain ICP, src/main.cpp:99-110): N ICP iterations (the reference iterates forever; default 50)
//   modes 3/4   (Go-ICP,   src/main.cpp:111-141): full registration
// Prints the result the way the reference logs it and writes io.output (output.toml) when set.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/goicp_mi355.hpp"

using namespace goicp_mi355;
struct P3 { float x, y, z; };

static std::string resolve(const std::string& p, const std::string& toml)
{
	if (p.empty() || p[0] == '/') return p;
	FILE* f = std::fopen(p.c_str(), "rb");
	if (f) { std::fclose(f); return p; }
	size_t s = toml.find_last_of("/\\");
	return s == std::string::npos ? p : toml.substr(0, s + 1) + p;
}

// path.ext -> path.k.ext (no extension: path.k)
static std::string numbered(const std::string& p, int k)
{
	const size_t slash = p.find_last_of("/\\"), dot = p.find_last_of('.');
	const std::string tag = "." + std::to_string(k);
	if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return p + tag;
	return p.substr(0, dot) + tag + p.substr(dot);
}

// goicp_cli --estimate-normals IN OUT.ply [--normal-k K] [--viewpoint X,Y,Z] [--verbose]: no config, no registration.  `at` is the
// position of --estimate-normals in argv
static int estimate_normals_mode(int argc, char** argv, int at)
{
	const char *in = at + 1 < argc ? argv[at + 1] : nullptr, *out = at + 2 < argc ? argv[at + 2] : nullptr;
	const char *k_arg = nullptr, *vp_arg = nullptr;
	int verbose = 0;
	// refused before any device is touched
	for (int i = 1; i < argc; i++) {
		if (i >= at && i <= at + 2) continue;
		if (!std::strcmp(argv[i], "--ranks")) {
			std::fprintf(stderr, "error: --estimate-normals cannot be combined with --ranks (it runs on one device and registers nothing)\n");
			return 2;
		}
		if (!std::strcmp(argv[i], "--normal-k")) k_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--viewpoint")) vp_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--verbose")) verbose = 1;
		else {
			std::fprintf(stderr, "error: --estimate-normals takes --normal-k K, --viewpoint X,Y,Z and --verbose, got '%s'\n", argv[i]);
			return 2;
		}
	}
	if (!in || !out || !*in || !*out || !std::strncmp(in, "--", 2) || !std::strncmp(out, "--", 2)) {
		std::fprintf(stderr, "error: --estimate-normals needs IN and OUT.ply\n");
		return 2;
	}
	long k = 16;
	if (k_arg) {
		char* end = nullptr;
		k = std::strtol(k_arg, &end, 10);
		if (end == k_arg || *end != '\0' || k < 3 || k > GOICP_KNN_SELF_MAX) {
			std::fprintf(stderr, "error: --estimate-normals needs --normal-k in 3..%d, got '%s'\n", GOICP_KNN_SELF_MAX, k_arg);
			return 2;
		}
	}
	float vp[3] = {0.f, 0.f, 0.f};
	if (vp_arg) {
		const char* s = vp_arg;
		bool ok = true;
		for (int a = 0; a < 3 && ok; a++) {
			char* end = nullptr;
			vp[a] = std::strtof(s, &end);
			ok = end != s && std::isfinite(vp[a]) && *end == (a < 2 ? ',' : '\0');
			s = end + 1;
		}
		if (!ok) {
			std::fprintf(stderr, "error: --viewpoint needs three finite numbers X,Y,Z, got '%s'\n", vp_arg);
			return 2;
		}
	}
	try {
		std::vector<P3> cloud;
		load_cloud(in, 1.f, 1.f, cloud, 0);
		const size_t n = cloud.size();
		std::vector<float> normals(3 * n), variation(n);
		// a handle only lends its device: eight corners of a cube are its clouds
		std::vector<P3> corners;
		for (int c = 0; c < 8; c++) corners.push_back(P3{c & 1 ? 0.5f : -0.5f, c & 2 ? 0.5f : -0.5f, c & 4 ? 0.5f : -0.5f});
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 32;
		params.verbose = verbose;
		goicp_handle h = nullptr;
		const auto t0 = std::chrono::steady_clock::now();
		const int rc = goicp_create(&params, &corners[0].x, 8, &corners[0].x, 8, &h);
		if (rc != GOICP_OK && rc != GOICP_ERR_NO_DEVICE) check(rc);
		const auto t1 = std::chrono::steady_clock::now();
		const int st = h ? goicp_estimate_normals(h, &cloud[0].x, n, (int32_t)k, vp_arg ? vp : nullptr, normals.data(), variation.data(), nullptr)
		                 : goicp_estimate_normals_host(n ? &cloud[0].x : nullptr, n, (int32_t)k, vp_arg ? vp : nullptr, normals.data(), variation.data(), nullptr);
		const auto t2 = std::chrono::steady_clock::now();
		const std::string why = st != GOICP_OK ? goicp_last_error() : "";
		const bool on_device = h != nullptr;
		if (h) goicp_destroy(h);
		if (st != GOICP_OK) throw std::runtime_error(why);
		FILE* f = std::fopen(out, "w");
		if (!f) throw std::runtime_error(std::string("cannot write ") + out);
		std::fprintf(f, "ply\nformat ascii 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
		                "property float nz\nproperty float curvature\nend_header\n", n);
		for (size_t i = 0; i < n; i++)
			std::fprintf(f, "%.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", cloud[i].x, cloud[i].y, cloud[i].z, normals[3 * i], normals[3 * i + 1], normals[3 * i + 2],
			             variation[i]);
		if (std::fclose(f) != 0) throw std::runtime_error(std::string("cannot write ") + out);
		std::printf("estimate normals: %zu points, k %ld, %s, %.2f ms%s -> %s\n", n, k, on_device ? "on the device" : "on the host (no device)",
		            std::chrono::duration<double, std::milli>(t2 - t1).count(),
		            on_device ? (" (handle " + std::to_string(std::chrono::duration<double, std::milli>(t1 - t0).count()) + " ms)").c_str() : "", out);
		return 0;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
}

// goicp_cli --fpfh-match SRC TGT OUT.txt [--fpfh-k K] [--normal-k K] [--voxel V] [--verbose]: no config, no registration.  `at` is the
// position of --fpfh-match in argv
static int fpfh_match_mode(int argc, char** argv, int at)
{
	const char* path[3] = {at + 1 < argc ? argv[at + 1] : nullptr, at + 2 < argc ? argv[at + 2] : nullptr, at + 3 < argc ? argv[at + 3] : nullptr};
	const char *k_arg = nullptr, *nk_arg = nullptr, *voxel_arg = nullptr;
	int verbose = 0;
	// refused before any device is touched
	for (int i = 1; i < argc; i++) {
		if (i >= at && i <= at + 3) continue;
		if (!std::strcmp(argv[i], "--ranks")) {
			std::fprintf(stderr, "error: --fpfh-match cannot be combined with --ranks (it runs on one device and registers nothing)\n");
			return 2;
		}
		if (!std::strcmp(argv[i], "--fpfh-k")) k_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--normal-k")) nk_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--voxel")) voxel_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--verbose")) verbose = 1;
		else {
			std::fprintf(stderr, "error: --fpfh-match takes --fpfh-k K, --normal-k K, --voxel V and --verbose, got '%s'\n", argv[i]);
			return 2;
		}
	}
	for (int a = 0; a < 3; a++)
		if (!path[a] || !*path[a] || !std::strncmp(path[a], "--", 2)) {
			std::fprintf(stderr, "error: --fpfh-match needs SRC, TGT and OUT.txt\n");
			return 2;
		}
	long k = 16, nk = 16;
	for (int a = 0; a < 2; a++) {
		const char* arg = a ? nk_arg : k_arg;
		if (!arg) continue;
		char* end = nullptr;
		const long v = std::strtol(arg, &end, 10);
		if (end == arg || *end != '\0' || v < (a ? 3 : 1) || v > GOICP_KNN_SELF_MAX) {
			std::fprintf(stderr, "error: --fpfh-match needs %s in %d..%d, got '%s'\n", a ? "--normal-k" : "--fpfh-k", a ? 3 : 1, GOICP_KNN_SELF_MAX, arg);
			return 2;
		}
		(a ? nk : k) = v;
	}
	float voxel = 0.f;
	if (voxel_arg) {
		char* end = nullptr;
		voxel = std::strtof(voxel_arg, &end);
		if (end == voxel_arg || *end != '\0' || !(voxel > 0.f) || !(voxel <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: --voxel needs a finite voxel size > 0, got '%s'\n", voxel_arg);
			return 2;
		}
	}
	try {
		std::vector<P3> cloud[2];
		for (int c = 0; c < 2; c++) {
			load_cloud(path[c], 1.f, 1.f, cloud[c], 0);
			if (voxel_arg && !cloud[c].empty()) {
				std::vector<P3> cells(cloud[c].size());
				size_t m = 0;
				check(goicp_voxel_downsample_host(&cloud[c][0].x, cloud[c].size(), voxel, &cells[0].x, nullptr, &m));
				cells.resize(m);
				cloud[c].swap(cells);
			}
		}
		// a handle only lends its device: eight corners of a cube are its clouds
		std::vector<P3> corners;
		for (int c = 0; c < 8; c++) corners.push_back(P3{c & 1 ? 0.5f : -0.5f, c & 2 ? 0.5f : -0.5f, c & 4 ? 0.5f : -0.5f});
		goicp_params params;
		goicp_params_default(&params);
		params.dt_size = 32;
		params.verbose = verbose;
		goicp_handle h = nullptr;
		const int rc = goicp_create(&params, &corners[0].x, 8, &corners[0].x, 8, &h);
		if (rc != GOICP_OK && rc != GOICP_ERR_NO_DEVICE) check(rc);
		const bool on_device = h != nullptr;
		const auto t0 = std::chrono::steady_clock::now();
		std::vector<float> feature[2];
		int st = GOICP_OK;
		for (int c = 0; c < 2 && st == GOICP_OK; c++) {
			const size_t n = cloud[c].size();
			const float* xyz = n ? &cloud[c][0].x : nullptr;
			std::vector<float> normals(3 * n);
			feature[c].resize(n * (size_t)GOICP_FPFH_DIM);
			st = h ? goicp_estimate_normals(h, xyz, n, (int32_t)nk, nullptr, normals.data(), nullptr, nullptr)
			       : goicp_estimate_normals_host(xyz, n, (int32_t)nk, nullptr, normals.data(), nullptr, nullptr);
			if (st == GOICP_OK)
				st = h ? goicp_fpfh(h, xyz, normals.data(), n, (int32_t)k, feature[c].data(), nullptr)
				       : goicp_fpfh_host(xyz, normals.data(), n, (int32_t)k, feature[c].data(), nullptr);
		}
		const size_t nq = cloud[0].size(), nt = cloud[1].size();
		std::vector<int32_t> index(nq);
		std::vector<float> d2(nq), second(nq);
		std::vector<uint8_t> mutual(nq);
		if (st == GOICP_OK)
			st = h ? goicp_match_features(h, feature[0].data(), nq, feature[1].data(), nt, index.data(), d2.data(), second.data(), mutual.data())
			       : goicp_match_features_host(feature[0].data(), nq, feature[1].data(), nt, index.data(), d2.data(), second.data(), mutual.data());
		const auto t1 = std::chrono::steady_clock::now();
		const std::string why = st != GOICP_OK ? goicp_last_error() : "";
		if (h) goicp_destroy(h);
		if (st != GOICP_OK) throw std::runtime_error(why);
		FILE* f = std::fopen(path[2], "w");
		if (!f) throw std::runtime_error(std::string("cannot write ") + path[2]);
		size_t matches = 0;
		for (size_t i = 0; i < nq; i++)
			if (mutual[i]) {
				std::fprintf(f, "%zu %d %.9g %.9g\n", i, index[i], d2[i], second[i]);
				matches++;
			}
		if (std::fclose(f) != 0) throw std::runtime_error(std::string("cannot write ") + path[2]);
		std::printf("fpfh match: %zu x %zu points, k %ld, normal k %ld, %zu mutual matches, %s, %.2f ms -> %s\n", nq, nt, k, nk, matches,
		            on_device ? "on the device" : "on the host (no device)", std::chrono::duration<double, std::milli>(t1 - t0).count(), path[2]);
		return 0;
	} catch (const std::exception& e) {
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
}

int main(int argc, char** argv)
{
	for (int i = 1; i < argc; i++)
		if (!std::strcmp(argv[i], "--estimate-normals")) return estimate_normals_mode(argc, argv, i);
	for (int i = 1; i < argc; i++)
		if (!std::strcmp(argv[i], "--fpfh-match")) return fpfh_match_mode(argc, argv, i);
	if (argc < 2) { std::fprintf(stderr, "usage: goicp_cli <config.toml> [--iters N] [--trim-fraction F] [--verbose] [--seed S] [--ranks N] [--reference-root] [--point-to-plane] [--normal-k K] [--symmetric [--source-normal-k K]] [--generalized [--gicp-epsilon E]] [--max-corr-dist D] [--robust-kernel {huber,cauchy,gm,tukey} --robust-scale C] [--trunc-dist D] [--information [--information-rank-tol X]] [--source-list FILE] [--voxel V] [--target-voxel V] [--outlier-radius R --outlier-min-neighbors K] [--target-outlier-radius R --target-outlier-min-neighbors K] [--stat-neighbors K --stat-std-ratio A] [--target-stat-neighbors K --target-stat-std-ratio A] [--plane-distance D [--plane-iterations T] [--plane-max P] [--plane-min-inliers S] [--plane-seed X] [--plane-no-refine]] [--target-plane-distance D ...] [--feature-init [--feature-voxel V] [--fpfh-k K] [--match-ratio R] [--ransac-distance D] [--ransac-iterations T] [--ransac-poses K] [--ransac-seed X]]\n"); return 2; }
	int iters = 50, verbose = 0, ranks = 1, reference_root = 0, plane = 0, normal_k = 16, symmetric = 0, source_normal_k = 16, generalized = 0;
	float gicp_epsilon = 1e-3f;
	const char* snk_arg = nullptr;
	const char* geps_arg = nullptr;
	float trim_fraction = 0.f;   // the TOML's `trim = true` carries no fraction (the reference ignores it): given here
	unsigned long long seed = 0;
	const char* gate_arg = nullptr;
	float gate = 0.f;
	const char *rk_arg = nullptr, *rc_arg = nullptr;
	const char* trunc_arg = nullptr;
	float trunc = 0.f;
	int robust_kernel = 0;
	float robust_scale = 0.f;
	int information = 0;
	const char* rank_tol_arg = nullptr;
	double rank_tol = -1.0;
	const char* list_arg = nullptr;
	std::vector<std::string> source_list;
	const char *voxel_arg = nullptr, *tvoxel_arg = nullptr;
	float voxel = 0.f, target_voxel = 0.f;
	const char *orad_arg[2] = {nullptr, nullptr}, *omin_arg[2] = {nullptr, nullptr};   // [0] the source's, [1] the target's
	float outlier_radius[2] = {0.f, 0.f};
	int outlier_min[2] = {0, 0};
	const char *sk_arg[2] = {nullptr, nullptr}, *sa_arg[2] = {nullptr, nullptr};       // statistical filter: [0] the source's, [1] the target's
	int stat_k[2] = {0, 0};
	float stat_ratio[2] = {0.f, 0.f};
	const char* cl_arg[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};   // radius, min-neighbors, min-size, keep
	goicp_cluster_select cluster[2];                                                                        // [0] the source's, [1] the target's
	for (int k = 0; k < 2; k++) goicp_cluster_select_default(&cluster[k]);
	const char* pl_arg[2][5] = {{nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr}};   // distance, iterations, max, min-inliers, seed
	int pl_no_refine[2] = {0, 0};
	goicp_plane_select plane_sel[2];                                                                        // [0] the source's, [1] the target's
	for (int k = 0; k < 2; k++) goicp_plane_select_default(&plane_sel[k]);
	// --feature-init: the ICP of modes 0..2 starts from the best RANSAC pose over FPFH matches, not from the identity
	int feature_init = 0;
	const char* ft_arg[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // voxel, fpfh-k, match-ratio, ransac-distance, -iterations, -poses, -seed
	float feature_voxel = 0.f, match_ratio = 0.f;
	long fpfh_k = 16;
	goicp_ransac_pose_select ransac_sel;
	goicp_ransac_pose_select_default(&ransac_sel);
	for (int i = 2; i < argc; i++) {
		if (!std::strcmp(argv[i], "--iters") && i + 1 < argc) iters = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
		else if (!std::strcmp(argv[i], "--trim-fraction") && i + 1 < argc) trim_fraction = (float)std::atof(argv[++i]);
		else if (!std::strcmp(argv[i], "--verbose")) verbose = 1;
		else if (!std::strcmp(argv[i], "--ranks") && i + 1 < argc) ranks = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--reference-root")) reference_root = 1;
		else if (!std::strcmp(argv[i], "--point-to-plane")) plane = 1;
		else if (!std::strcmp(argv[i], "--normal-k") && i + 1 < argc) normal_k = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--symmetric")) symmetric = plane = 1;
		else if (!std::strcmp(argv[i], "--generalized")) generalized = plane = 1;
		else if (!std::strcmp(argv[i], "--gicp-epsilon")) geps_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--source-normal-k")) snk_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--max-corr-dist")) gate_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--robust-kernel")) rk_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--robust-scale")) rc_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--trunc-dist")) trunc_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--information")) information = 1;
		else if (!std::strcmp(argv[i], "--information-rank-tol")) rank_tol_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--source-list")) list_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--voxel")) voxel_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--target-voxel")) tvoxel_arg = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--outlier-radius")) orad_arg[0] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--outlier-min-neighbors")) omin_arg[0] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--target-outlier-radius")) orad_arg[1] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--target-outlier-min-neighbors")) omin_arg[1] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--stat-neighbors")) sk_arg[0] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--stat-std-ratio")) sa_arg[0] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--target-stat-neighbors")) sk_arg[1] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--target-stat-std-ratio")) sa_arg[1] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--feature-init")) feature_init = 1;
		else if (!std::strcmp(argv[i], "--feature-voxel")) ft_arg[0] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--fpfh-k")) ft_arg[1] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--match-ratio")) ft_arg[2] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--ransac-distance")) ft_arg[3] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--ransac-iterations")) ft_arg[4] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--ransac-poses")) ft_arg[5] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--ransac-seed")) ft_arg[6] = i + 1 < argc ? argv[++i] : "";
		else if (!std::strcmp(argv[i], "--plane-no-refine")) pl_no_refine[0] = 1;
		else if (!std::strcmp(argv[i], "--target-plane-no-refine")) pl_no_refine[1] = 1;
		else {
			static const char* const cl_names[2][4] = {{"--cluster-radius", "--cluster-min-neighbors", "--cluster-min-size", "--cluster-keep"},
			                                           {"--target-cluster-radius", "--target-cluster-min-neighbors", "--target-cluster-min-size", "--target-cluster-keep"}};
			const char* const name = argv[i];                       // a match below consumes the value after it
			for (int q = 0; q < 8; q++)
				if (!std::strcmp(name, cl_names[q / 4][q % 4])) { cl_arg[q / 4][q % 4] = i + 1 < argc ? argv[++i] : ""; break; }
			static const char* const pl_names[2][5] = {{"--plane-distance", "--plane-iterations", "--plane-max", "--plane-min-inliers", "--plane-seed"},
			                                           {"--target-plane-distance", "--target-plane-iterations", "--target-plane-max", "--target-plane-min-inliers",
			                                            "--target-plane-seed"}};
			for (int q = 0; q < 10; q++)
				if (!std::strcmp(name, pl_names[q / 5][q % 5])) { pl_arg[q / 5][q % 5] = i + 1 < argc ? argv[++i] : ""; break; }
		}
	}
	{
		// bad feature options are refused before any device is touched
		static const char* const ft_names[7] = {"--feature-voxel", "--fpfh-k", "--match-ratio", "--ransac-distance", "--ransac-iterations", "--ransac-poses",
		                                        "--ransac-seed"};
		for (int q = 0; q < 7; q++) {
			if (!ft_arg[q]) continue;
			if (!feature_init) {
				std::fprintf(stderr, "error: %s needs --feature-init\n", ft_names[q]);
				return 2;
			}
			char* end = nullptr;
			bool ok = true;
			if (q == 0 || q == 2 || q == 3) {
				const float v = std::strtof(ft_arg[q], &end);
				ok = end != ft_arg[q] && *end == '\0' && v <= 3.402823466e+38f && (q == 2 ? v >= 0.f : v > 0.f);
				(q == 0 ? feature_voxel : (q == 2 ? match_ratio : ransac_sel.distance)) = v;
			} else if (q == 6) {
				ransac_sel.seed = std::strtoull(ft_arg[q], &end, 10);
				ok = end != ft_arg[q] && *end == '\0';
			} else {
				const long v = std::strtol(ft_arg[q], &end, 10);
				const long hi = q == 1 ? GOICP_KNN_SELF_MAX : (q == 4 ? GOICP_RANSAC_POSE_MAX_ITERATIONS : GOICP_RANSAC_POSE_MAX_POSES);
				ok = end != ft_arg[q] && *end == '\0' && v >= 1 && v <= hi;
				if (q == 1) fpfh_k = v;
				else (q == 4 ? ransac_sel.iterations : ransac_sel.max_poses) = (int32_t)v;
			}
			if (!ok) {
				std::fprintf(stderr, "error: %s got a value out of range: '%s'\n", ft_names[q], ft_arg[q]);
				return 2;
			}
		}
		if (feature_init && !ft_arg[3]) {
			if (!ft_arg[0]) {
				std::fprintf(stderr, "error: --feature-init needs --ransac-distance D or --feature-voxel V (D = 1.5 V)\n");
				return 2;
			}
			ransac_sel.distance = 1.5f * feature_voxel;
		}
		if (feature_init && (normal_k < 3 || normal_k > GOICP_KNN_SELF_MAX)) {
			std::fprintf(stderr, "error: --feature-init needs --normal-k in 3..%d\n", GOICP_KNN_SELF_MAX);
			return 2;
		}
		if (feature_init && (ranks > 1 || list_arg)) {
			std::fprintf(stderr, "error: --feature-init cannot be combined with --ranks or --source-list\n");
			return 2;
		}
	}
	for (int k = 0; k < 2; k++) {
		// a bad voxel is refused before any device is touched
		const char* arg = k ? tvoxel_arg : voxel_arg;
		if (!arg) continue;
		char* end = nullptr;
		const float v = std::strtof(arg, &end);
		if (end == arg || *end != '\0' || !(v > 0.f) || !(v <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: %s needs a finite voxel size > 0, got '%s'\n", k ? "--target-voxel" : "--voxel", arg);
			return 2;
		}
		(k ? target_voxel : voxel) = v;
	}
	for (int k = 0; k < 2; k++) {
		// a bad outlier filter is refused before any device is touched
		const char* pre = k ? "--target-outlier" : "--outlier";
		if (!orad_arg[k] && !omin_arg[k]) continue;
		if (!orad_arg[k] || !omin_arg[k]) {
			std::fprintf(stderr, "error: %s-radius and %s-min-neighbors go together\n", pre, pre);
			return 2;
		}
		char* end = nullptr;
		const float r = std::strtof(orad_arg[k], &end);
		const float r2 = r * r;
		if (end == orad_arg[k] || *end != '\0' || !(r > 0.f) || !(r2 >= 1.17549435e-38f) || !(r2 <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: %s-radius needs a finite radius > 0 whose square is a normal float, got '%s'\n", pre, orad_arg[k]);
			return 2;
		}
		const long kk = std::strtol(omin_arg[k], &end, 10);
		if (end == omin_arg[k] || *end != '\0' || kk < 1 || kk > 2147483647L) {
			std::fprintf(stderr, "error: %s-min-neighbors needs an integer >= 1, got '%s'\n", pre, omin_arg[k]);
			return 2;
		}
		outlier_radius[k] = r;
		outlier_min[k] = (int)kk;
	}
	for (int k = 0; k < 2; k++) {
		// a bad statistical filter is refused before any device is touched
		const char* pre = k ? "--target-stat" : "--stat";
		if (!sk_arg[k] && !sa_arg[k]) continue;
		if (!sk_arg[k] || !sa_arg[k]) {
			std::fprintf(stderr, "error: %s-neighbors and %s-std-ratio go together\n", pre, pre);
			return 2;
		}
		char* end = nullptr;
		const long kk = std::strtol(sk_arg[k], &end, 10);
		if (end == sk_arg[k] || *end != '\0' || kk < 1 || kk > GOICP_STAT_MAX_NEIGHBORS) {
			std::fprintf(stderr, "error: %s-neighbors needs an integer in 1..%d, got '%s'\n", pre, GOICP_STAT_MAX_NEIGHBORS, sk_arg[k]);
			return 2;
		}
		const float a = std::strtof(sa_arg[k], &end);
		if (end == sa_arg[k] || *end != '\0' || !(a >= 0.f) || !(a <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: %s-std-ratio needs a finite number >= 0, got '%s'\n", pre, sa_arg[k]);
			return 2;
		}
		stat_k[k] = (int)kk;
		stat_ratio[k] = a;
	}
	for (int k = 0; k < 2; k++) {
		// a bad cluster selection is refused before any device is touched
		const char* pre = k ? "--target-cluster" : "--cluster";
		if (!cl_arg[k][0] && !cl_arg[k][1] && !cl_arg[k][2] && !cl_arg[k][3]) continue;
		if (!cl_arg[k][0]) {
			std::fprintf(stderr, "error: %s-min-neighbors, %s-min-size and %s-keep need %s-radius\n", pre, pre, pre, pre);
			return 2;
		}
		char* end = nullptr;
		const float r = std::strtof(cl_arg[k][0], &end);
		const float r2 = r * r;
		if (end == cl_arg[k][0] || *end != '\0' || !(r > 0.f) || !(r2 >= 1.17549435e-38f) || !(r2 <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: %s-radius needs a finite radius > 0 whose square is a normal float, got '%s'\n", pre, cl_arg[k][0]);
			return 2;
		}
		static const char* const what[4] = {"radius", "min-neighbors", "min-size", "keep"};
		long v[4] = {0, 0, 0, 1};                                   // the defaults: every point is core, any size, the largest cluster
		for (int a = 1; a < 4; a++) {
			if (!cl_arg[k][a]) continue;
			v[a] = std::strtol(cl_arg[k][a], &end, 10);
			if (end == cl_arg[k][a] || *end != '\0' || v[a] < 0 || v[a] > 2147483647L) {
				std::fprintf(stderr, "error: %s-%s needs an integer >= 0, got '%s'\n", pre, what[a], cl_arg[k][a]);
				return 2;
			}
		}
		cluster[k].radius = r;
		cluster[k].min_neighbors = (int32_t)v[1]; cluster[k].min_size = (int32_t)v[2]; cluster[k].max_clusters = (int32_t)v[3];
	}
	for (int k = 0; k < 2; k++) {
		// a bad plane selection is refused before any device is touched
		const char* pre = k ? "--target-plane" : "--plane";
		if (!pl_arg[k][0] && !pl_arg[k][1] && !pl_arg[k][2] && !pl_arg[k][3] && !pl_arg[k][4] && !pl_no_refine[k]) continue;
		if (!pl_arg[k][0]) {
			std::fprintf(stderr, "error: %s-iterations, %s-max, %s-min-inliers, %s-seed and %s-no-refine need %s-distance\n", pre, pre, pre, pre, pre, pre);
			return 2;
		}
		char* end = nullptr;
		const float d = std::strtof(pl_arg[k][0], &end);
		if (end == pl_arg[k][0] || *end != '\0' || !(d > 0.f) || !(d <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: %s-distance needs a finite distance > 0, got '%s'\n", pre, pl_arg[k][0]);
			return 2;
		}
		static const char* const what[4] = {"distance", "iterations", "max", "min-inliers"};
		const long top[4] = {0, GOICP_PLANE_MAX_ITERATIONS, GOICP_PLANE_MAX_PLANES, 2147483647L};
		long v[4] = {0, 0, 0, 0};                                   // the defaults: 1000 hypotheses, one plane, any count
		for (int a = 1; a < 4; a++) {
			if (!pl_arg[k][a]) continue;
			v[a] = std::strtol(pl_arg[k][a], &end, 10);
			if (end == pl_arg[k][a] || *end != '\0' || v[a] < 0 || v[a] > top[a]) {
				std::fprintf(stderr, "error: %s-%s needs an integer in 0..%ld, got '%s'\n", pre, what[a], top[a], pl_arg[k][a]);
				return 2;
			}
		}
		unsigned long long sd = 0;
		if (pl_arg[k][4]) {
			sd = std::strtoull(pl_arg[k][4], &end, 10);
			if (end == pl_arg[k][4] || *end != '\0' || pl_arg[k][4][0] == '-') {
				std::fprintf(stderr, "error: %s-seed needs an unsigned integer, got '%s'\n", pre, pl_arg[k][4]);
				return 2;
			}
		}
		plane_sel[k].distance = d;
		plane_sel[k].iterations = (int32_t)v[1]; plane_sel[k].max_planes = (int32_t)v[2]; plane_sel[k].min_inliers = (int32_t)v[3];
		plane_sel[k].refine = pl_no_refine[k] ? 0 : 1;
		plane_sel[k].seed = (uint64_t)sd;
	}
	if (list_arg) {
		// refused before any device is touched
		if (ranks > 1) {
			std::fprintf(stderr, "error: --source-list cannot be combined with --ranks N > 1 (the multi-GPU registration creates its own engines)\n");
			return 2;
		}
		FILE* f = *list_arg ? std::fopen(list_arg, "r") : nullptr;
		if (!f) {
			std::fprintf(stderr, "error: --source-list needs a readable file with one cloud path per line, got '%s'\n", list_arg);
			return 2;
		}
		char line[4096];
		while (std::fgets(line, sizeof(line), f)) {
			std::string s(line);
			while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ' || s.back() == '\t')) s.pop_back();
			size_t b = 0;
			while (b < s.size() && (s[b] == ' ' || s[b] == '\t')) b++;
			s = s.substr(b);
			if (!s.empty() && s[0] != '#') source_list.push_back(resolve(s, list_arg));
		}
		std::fclose(f);
		if (source_list.empty()) {
			std::fprintf(stderr, "error: --source-list: '%s' names no cloud\n", list_arg);
			return 2;
		}
	}
	if (rk_arg || rc_arg) {
		// a bad robust kernel is refused before any device is touched
		static const char* const names[4] = {"huber", "cauchy", "gm", "tukey"};
		for (int k = 0; rk_arg && k < 4; k++)
			if (!std::strcmp(rk_arg, names[k])) robust_kernel = k + 1;
		if (!robust_kernel) {
			std::fprintf(stderr, "error: --robust-kernel needs one of huber, cauchy, gm, tukey (and --robust-scale needs --robust-kernel), got '%s'\n", rk_arg ? rk_arg : "");
			return 2;
		}
		char* end = nullptr;
		robust_scale = rc_arg ? std::strtof(rc_arg, &end) : 0.f;
		if (!rc_arg || end == rc_arg || *end != '\0' || !(robust_scale > 0.f) || !(robust_scale <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: --robust-kernel needs --robust-scale with a finite scale > 0, got '%s'\n", rc_arg ? rc_arg : "");
			return 2;
		}
		if (ranks > 1 || trim_fraction > 0.f || gate_arg) {
			std::fprintf(stderr, "error: --robust-kernel cannot be combined with --ranks N > 1 (the multi-GPU registration is plain), --trim-fraction F > 0 or --max-corr-dist\n");
			return 2;
		}
	}
	if (gate_arg) {
		// a bad gate is refused before any device is touched
		char* end = nullptr;
		gate = std::strtof(gate_arg, &end);
		if (end == gate_arg || *end != '\0' || !(gate > 0.f) || !(gate <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: --max-corr-dist needs a finite distance > 0, got '%s'\n", gate_arg);
			return 2;
		}
		if (ranks > 1 || trim_fraction > 0.f) {
			std::fprintf(stderr, "error: --max-corr-dist cannot be combined with --ranks N > 1 (the multi-GPU registration is ungated) or --trim-fraction F > 0\n");
			return 2;
		}
	}
	if (trunc_arg) {
		// a bad truncation distance is refused before any device is touched
		char* end = nullptr;
		trunc = std::strtof(trunc_arg, &end);
		if (end == trunc_arg || *end != '\0' || !(trunc > 0.f) || !(trunc <= 3.402823466e+38f)) {
			std::fprintf(stderr, "error: --trunc-dist needs a finite distance > 0, got '%s'\n", trunc_arg);
			return 2;
		}
		if (ranks > 1 || trim_fraction > 0.f) {
			std::fprintf(stderr, "error: --trunc-dist cannot be combined with --ranks N > 1 (the multi-GPU registration searches the plain objective) or --trim-fraction F > 0\n");
			return 2;
		}
	}
	if (information || rank_tol_arg) {
		// refused before any device is touched
		if (!information) {
			std::fprintf(stderr, "error: --information-rank-tol needs --information\n");
			return 2;
		}
		if (rank_tol_arg) {
			char* end = nullptr;
			rank_tol = std::strtod(rank_tol_arg, &end);
			if (end == rank_tol_arg || *end != '\0' || !(rank_tol >= 0.0 && rank_tol < 1.0)) {
				std::fprintf(stderr, "error: --information-rank-tol needs a number in [0, 1), got '%s'\n", rank_tol_arg);
				return 2;
			}
		}
		if (ranks > 1) {
			std::fprintf(stderr, "error: --information cannot be combined with --ranks N > 1 (the multi-GPU registration has no information pass)\n");
			return 2;
		}
	}
	if (snk_arg) {
		char* end = nullptr;
		const long k = std::strtol(snk_arg, &end, 10);
		if (end == snk_arg || *end != '\0' || k < 3 || k > GOICP_KNN_SELF_MAX) {
			std::fprintf(stderr, "error: --source-normal-k needs an integer in 3..%d, got '%s'\n", GOICP_KNN_SELF_MAX, snk_arg);
			return 2;
		}
		if (!symmetric && !generalized) {
			std::fprintf(stderr, "error: --source-normal-k goes with --symmetric or --generalized\n");
			return 2;
		}
		source_normal_k = (int)k;
	}
	if (symmetric && (ranks > 1 || trim_fraction > 0.f)) {
		std::fprintf(stderr, "error: --symmetric cannot be combined with --ranks N > 1 (the multi-GPU registration runs point-to-point ICP) or --trim-fraction F > 0\n");
		return 2;
	}
	if (geps_arg) {
		char* end = nullptr;
		const float e = std::strtof(geps_arg, &end);
		if (end == geps_arg || *end != '\0' || !(e >= 1e-4f && e <= 1.f)) {
			std::fprintf(stderr, "error: --gicp-epsilon needs a number in [1e-4, 1], got '%s'\n", geps_arg);
			return 2;
		}
		if (!generalized) {
			std::fprintf(stderr, "error: --gicp-epsilon goes with --generalized\n");
			return 2;
		}
		gicp_epsilon = e;
	}
	if (generalized && (symmetric || ranks > 1 || trim_fraction > 0.f)) {
		std::fprintf(stderr, "error: --generalized cannot be combined with --symmetric, --ranks N > 1 (the multi-GPU registration runs point-to-point ICP) or --trim-fraction F > 0\n");
		return 2;
	}
	if (plane && ranks > 1) {
		// the multi-GPU registration runs point-to-point ICP only: refused before any device is touched
		std::fprintf(stderr, "error: --point-to-plane cannot be combined with --ranks N > 1 (the multi-GPU registration runs point-to-point ICP)\n");
		return 2;
	}
	try {
		Config config(argv[1]);
		// refused before any device is touched: the result files report the engine's own search and ICP state, which a run from a feature pose
		// does not set, and modes 3/4 search globally and take no start pose
		if (feature_init && config.mode > 2) throw std::runtime_error("--feature-init starts the ICP of modes 0..2; modes 3/4 search globally and take no start pose");
		if (feature_init && (!config.io.output.empty() || !config.io.visualization.empty()))
			throw std::runtime_error("--feature-init cannot be combined with [io] output or visualization: the pose is printed, not written");
		std::vector<P3> source, target;
		load_cloud(resolve(config.io.source, argv[1]), config.subsample, config.resize, source, seed);
		load_cloud(resolve(config.io.target, argv[1]), config.subsample, config.resize, target, seed);
		for (int k = 0; k < 2; k++) {
			// the host function: no engine exists yet
			std::vector<P3>& cloud = k ? target : source;
			const float v = k ? target_voxel : voxel;
			if (!(v > 0.f) || cloud.empty()) continue;
			std::vector<P3> reduced(cloud.size());
			size_t m = 0;
			check(goicp_voxel_downsample_host(&cloud[0].x, cloud.size(), v, &reduced[0].x, nullptr, &m));
			reduced.resize(m);
			std::printf("%s voxel %g: %zu of %zu points kept\n", k ? "target" : "source", v, m, cloud.size());
			cloud.swap(reduced);
		}
		for (int k = 0; k < 2; k++) {
			// after the voxel grid, before the radius filter; the host function again
			std::vector<P3>& cloud = k ? target : source;
			if (stat_k[k] < 1 || cloud.empty()) continue;
			std::vector<P3> kept(cloud.size());
			size_t m = 0;
			check(goicp_statistical_outlier_removal_host(&cloud[0].x, cloud.size(), stat_k[k], stat_ratio[k], &kept[0].x, nullptr, nullptr, nullptr, &m));
			kept.resize(m);
			std::printf("%s stat neighbors %d std ratio %g: kept %zu of %zu points\n", k ? "target" : "source", stat_k[k], stat_ratio[k], m, cloud.size());
			cloud.swap(kept);
		}
		for (int k = 0; k < 2; k++) {
			// after the voxel grid and the statistical filter; the host function again
			std::vector<P3>& cloud = k ? target : source;
			if (!(outlier_radius[k] > 0.f) || cloud.empty()) continue;
			std::vector<P3> kept(cloud.size());
			size_t m = 0;
			check(goicp_radius_outlier_removal_host(&cloud[0].x, cloud.size(), outlier_radius[k], outlier_min[k], &kept[0].x, nullptr, nullptr, &m));
			kept.resize(m);
			std::printf("%s outlier radius %g min neighbors %d: kept %zu of %zu points\n", k ? "target" : "source", outlier_radius[k], outlier_min[k], m,
			            cloud.size());
			if (m == 0) throw std::runtime_error(std::string(k ? "target" : "source") + ": the outlier filter keeps no point");
			cloud.swap(kept);
		}
		for (int k = 0; k < 2; k++) {
			// after the neighbourhood filters, before the cluster selection; the host function again
			std::vector<P3>& cloud = k ? target : source;
			if (!(plane_sel[k].distance > 0.f) || cloud.empty()) continue;
			std::vector<P3> kept(cloud.size());
			goicp_plane found[GOICP_PLANE_MAX_PLANES];
			size_t m = 0, np = 0;
			check(goicp_plane_filter_host(&cloud[0].x, cloud.size(), &plane_sel[k], &kept[0].x, nullptr, found, &np, &m));
			kept.resize(m);
			std::printf("%s plane distance %g iterations %d max %d min inliers %d refine %d: %zu planes, kept %zu of %zu points\n", k ? "target" : "source",
			            plane_sel[k].distance, (int)plane_sel[k].iterations, (int)plane_sel[k].max_planes, (int)plane_sel[k].min_inliers, (int)plane_sel[k].refine, np, m,
			            cloud.size());
			for (size_t q = 0; q < np; q++)
				std::printf("%s plane %zu: %.9g x + %.9g y + %.9g z + %.9g = 0, %d inliers\n", k ? "target" : "source", q, found[q].normal[0], found[q].normal[1],
				            found[q].normal[2], found[q].d, (int)found[q].inliers);
			if (m == 0) throw std::runtime_error(std::string(k ? "target" : "source") + ": the plane removal keeps no point");
			cloud.swap(kept);
		}
		for (int k = 0; k < 2; k++) {
			// after every other filter; the host function again
			std::vector<P3>& cloud = k ? target : source;
			if (!(cluster[k].radius > 0.f) || cloud.empty()) continue;
			std::vector<P3> kept(cloud.size());
			size_t m = 0;
			check(goicp_cluster_filter_host(&cloud[0].x, cloud.size(), &cluster[k], &kept[0].x, nullptr, nullptr, &m));
			kept.resize(m);
			std::printf("%s cluster radius %g min neighbors %d min size %d keep %d: kept %zu of %zu points\n", k ? "target" : "source", cluster[k].radius,
			            (int)cluster[k].min_neighbors, (int)cluster[k].min_size, (int)cluster[k].max_clusters, m, cloud.size());
			if (m == 0) throw std::runtime_error(std::string(k ? "target" : "source") + ": the cluster selection keeps no point");
			cloud.swap(kept);
		}
		std::printf("mode %d: source %zu points, target %zu points, mse_threshold %g\n", config.mode, source.size(),
		            target.size(), config.mse_threshold);
		goicp_params p;
		goicp_params_from_config(&config.raw, &p);      // mse_threshold + the [params.rotation] / [params.translation] search ranges
		p.verbose = verbose;
		p.trim_fraction = trim_fraction;
		if (reference_root) { p.use_rot_range = 0; p.use_trans_range = 0; p.rot_search_depth = 0; p.trans_search_depth = 0; }
		if (ranks > 1 && config.mode > 2) {
			// the sharded search: one engine per GPU inside the library, rank 0's engine comes back for the result
			p.mse_threshold = config.mse_threshold;
			std::vector<goicp_shard_stats> st((size_t)ranks);
			goicp_handle h0 = nullptr;
			check(goicp_register_multi_gpu(&p, &target[0].x, target.size(), &source[0].x, source.size(), ranks, 8, &h0, st.data()));
			goicp_result r;
			check(goicp_poll(h0, &r));
			float sse_thr = 0.f; int32_t inliers = (int32_t)source.size();
			check(goicp_thresholds(h0, &sse_thr, &inliers));         // MSE over the inliers, as output.toml (jly_goicp.cpp:198-208)
			std::printf("Searching over (%d GPUs)! Best Error: %.7g  (MSE %.7g)\n", ranks, r.best_sse, r.best_sse / (float)inliers);
			for (int k = 0; k < ranks; k++)
				std::printf("rank %d: %lld steps (%lld idle), %lld exchanges, %lld pose broadcasts, %lld donations (%lld cubes), step %.1f ms, waiting in collectives %.1f ms\n",
				            k, (long long)st[(size_t)k].steps, (long long)st[(size_t)k].steps_idle, (long long)st[(size_t)k].exchanges, (long long)st[(size_t)k].broadcasts,
				            (long long)st[(size_t)k].donations, (long long)st[(size_t)k].donated_cubes, st[(size_t)k].step_ms, st[(size_t)k].wait_ms);
			std::printf("Optimal Rotation Matrix:\n");
			for (int i = 0; i < 3; i++) std::printf("%12.7f %12.7f %12.7f\n", r.optR[3 * i], r.optR[3 * i + 1], r.optR[3 * i + 2]);
			std::printf("Optimal Translation Vector:\n%12.7f\n%12.7f\n%12.7f\n", r.optT[0], r.optT[1], r.optT[2]);
			if (!config.io.output.empty()) check(goicp_result_write_toml(h0, config.io.output.c_str()));
			if (!config.io.visualization.empty()) check(goicp_result_write_ply(h0, config.io.visualization.c_str()));
			goicp_destroy(h0);
			return 0;
		}
		std::mutex mtx;
		icp::FastGoICP engine(target, source, config.mse_threshold, mtx, &p);
		goicp_handle h = engine.registration.handle();
		if (plane || (normal_k != 16 && !feature_init)) engine.registration.set_icp_options(plane, normal_k);   // with --feature-init alone --normal-k is the features' k
		if (symmetric) engine.registration.set_icp_symmetric(true, source_normal_k);
		if (generalized) engine.registration.set_icp_generalized(true, gicp_epsilon, source_normal_k);
		if (gate > 0.f) engine.registration.set_icp_gate(gate);
		if (robust_kernel) engine.registration.set_icp_robust(robust_kernel, robust_scale);
		if (trunc > 0.f) engine.registration.set_search_truncation(trunc);
		goicp_result r;
		if (feature_init) {
			// voxel grid -> normals -> FPFH -> matches -> correspondences -> RANSAC poses, on the device through the engine's handle
			std::vector<P3> cloud[2] = {source, target};
			std::vector<float> feature[2];
			for (int c = 0; c < 2; c++) {
				if (feature_voxel > 0.f) {
					std::vector<P3> cells(cloud[c].size());
					size_t m = 0;
					check(goicp_voxel_downsample(h, &cloud[c][0].x, cloud[c].size(), feature_voxel, &cells[0].x, nullptr, &m));
					cells.resize(m);
					cloud[c].swap(cells);
				}
				const size_t n = cloud[c].size();
				std::vector<float> normals(3 * n);
				feature[c].resize(n * (size_t)GOICP_FPFH_DIM);
				check(goicp_estimate_normals(h, &cloud[c][0].x, n, (int32_t)normal_k, nullptr, normals.data(), nullptr, nullptr));
				check(goicp_fpfh(h, &cloud[c][0].x, normals.data(), n, (int32_t)fpfh_k, feature[c].data(), nullptr));
			}
			const size_t nq = cloud[0].size(), nt = cloud[1].size();
			std::vector<int32_t> index(nq), corr(2 * nq);
			std::vector<float> d2(nq), second(nq);
			std::vector<uint8_t> mutual(nq);
			check(goicp_match_features(h, feature[0].data(), nq, feature[1].data(), nt, index.data(), d2.data(), second.data(), mutual.data()));
			size_t M = 0, found = 0;
			check(goicp_select_matches(index.data(), d2.data(), second.data(), mutual.data(), nq, match_ratio, 1, corr.data(), &M));
			std::vector<goicp_ransac_pose_result> poses(GOICP_RANSAC_POSE_MAX_POSES);
			if (M >= 3) check(goicp_ransac_pose(h, &cloud[0][0].x, nq, &cloud[1][0].x, nt, corr.data(), M, &ransac_sel, poses.data(), &found, nullptr));
			std::printf("feature init: %zu x %zu points, fpfh k %ld, normal k %d, ratio %g: %zu correspondences; ransac distance %g iterations %d: %zu poses", nq, nt,
			            fpfh_k, normal_k, match_ratio, M, ransac_sel.distance, (int)(ransac_sel.iterations ? ransac_sel.iterations : 100000), found);
			if (found) std::printf(", the best with %d inliers%s\n", (int)poses[0].inliers, poses[0].refined ? " (refit)" : "");
			else std::printf("\n");
			if (!found) throw std::runtime_error("--feature-init: the feature matches support no pose");
			float err = 0.f;
			int32_t done = 0;
			check(goicp_icp_run(h, poses[0].R, poses[0].t, iters, 0.f, &err, &done));
			check(goicp_poll(h, &r));
			std::memcpy(r.curR, poses[0].R, sizeof(r.curR)); std::memcpy(r.curT, poses[0].t, sizeof(r.curT));
			r.best_sse = err;
			std::printf("ICP from the feature pose after %d iterations: SSE %.7g\n", (int)done, err);
		} else if (config.mode <= 2) {
			for (int i = 0; i < iters; i++) check(goicp_icp_step(h));
			check(goicp_poll(h, &r));
			std::printf("ICP after %d iterations: SSE %.7g\n", iters, r.best_sse);
		} else {
			engine.run();
			check(goicp_poll(h, &r));
			float sse_thr = 0.f; int32_t inliers = (int32_t)source.size();
			check(goicp_thresholds(h, &sse_thr, &inliers));          // MSE over the inliers, as output.toml (jly_goicp.cpp:198-208)
			std::printf("Searching over! Best Error: %.7g  (MSE %.7g)\n", r.best_sse, r.best_sse / (float)inliers);
			std::printf("Total Translation Nodes Searched: %lld\nTotal Rotation Nodes Searched: %lld\n",
			            (long long)r.counters.trans_pops, (long long)r.counters.rot_pops);
			std::printf("cube bounds %lld in %.1f ms (DT build %.1f ms)\n", (long long)r.counters.cubes, r.register_ms, r.dt_build_ms);
		}
		const float* R = config.mode <= 2 ? r.curR : r.optR;
		const float* t = config.mode <= 2 ? r.curT : r.optT;
		std::printf("Optimal Rotation Matrix:\n");
		for (int i = 0; i < 3; i++) std::printf("%12.7f %12.7f %12.7f\n", R[3 * i], R[3 * i + 1], R[3 * i + 2]);
		std::printf("Optimal Translation Vector:\n%12.7f\n%12.7f\n%12.7f\n", t[0], t[1], t[2]);
		if (!config.io.output.empty()) engine.write_output(config.io.output);
		if (symmetric) {
			std::printf("ICP metric: symmetric point-to-plane (normal_k %d, source_normal_k %d)\n", normal_k, source_normal_k);
			if (!config.io.output.empty()) {
				FILE* f = std::fopen(config.io.output.c_str(), "a");
				if (!f) throw std::runtime_error("cannot append to " + config.io.output);
				std::fprintf(f, "\n[icp_symmetric]\nenabled = true\nsource_normal_k = %d\n", source_normal_k);
				std::fclose(f);
			}
		}
		if (generalized) {
			std::printf("ICP metric: generalized plane-to-plane (epsilon %.7g, normal_k %d, source_normal_k %d)\n", gicp_epsilon, normal_k, source_normal_k);
			if (!config.io.output.empty()) {
				FILE* f = std::fopen(config.io.output.c_str(), "a");
				if (!f) throw std::runtime_error("cannot append to " + config.io.output);
				std::fprintf(f, "\n[icp_generalized]\nenabled = true\nepsilon = %.9g\nsource_normal_k = %d\n", gicp_epsilon, source_normal_k);
				std::fclose(f);
			}
		}
		if (gate > 0.f) {
			int32_t n_in = 0;
			check(goicp_eval_correspondences(h, R, t, gate, nullptr, nullptr, &n_in, nullptr));
			std::printf("Inliers within %.7g: %d of %zu\n", gate, (int)n_in, source.size());
			if (!config.io.output.empty()) {
				FILE* f = std::fopen(config.io.output.c_str(), "a");
				if (!f) throw std::runtime_error("cannot append to " + config.io.output);
				std::fprintf(f, "\n[icp_gate]\nmax_corr_dist = %.9g\ninliers = %d\n", gate, (int)n_in);
				std::fclose(f);
			}
		}
		if (trunc > 0.f && !config.io.output.empty()) {
			FILE* f = std::fopen(config.io.output.c_str(), "a");
			if (!f) throw std::runtime_error("cannot append to " + config.io.output);
			std::fprintf(f, "\n[search]\ntrunc_dist = %.9g\n", trunc);
			std::fclose(f);
		}
		if (information) {
			goicp_pose_info_options io;
			goicp_pose_info_options_default(&io);
			if (rank_tol >= 0.0) io.rank_tol = rank_tol;
			const goicp_pose_info I = engine.registration.pose_information(R, t, &io);
			std::printf("Information: rank %d of 6, sigma %.7g (metric %d%s, %lld inliers)\n", (int)I.rank, std::sqrt(I.sigma2), (int)I.metric,
			            symmetric && I.metric == 1 ? " symmetric" : generalized && I.metric == 1 ? " generalized" : "", (long long)I.inliers);
			if (!config.io.output.empty()) {
				FILE* f = std::fopen(config.io.output.c_str(), "a");
				if (!f) throw std::runtime_error("cannot append to " + config.io.output);
				std::fprintf(f, "\n[information]\nmetric = %d\nrank = %d\nrank_tol = %.17g\nsigma2 = %.17g\ninliers = %lld\nweight_sum = %.17g\n", (int)I.metric, (int)I.rank,
				             io.rank_tol, I.sigma2, (long long)I.inliers, I.weight_sum);
				std::fprintf(f, "eigenvalues = [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g]\n", I.eigenvalues[0], I.eigenvalues[1], I.eigenvalues[2], I.eigenvalues[3],
				             I.eigenvalues[4], I.eigenvalues[5]);
				const double* mats[2] = {I.information, I.covariance};
				const char* names[2] = {"information", "covariance"};
				for (int m = 0; m < 2; m++) {
					std::fprintf(f, "%s = [\n", names[m]);
					for (int i = 0; i < 6; i++) {
						const double* row = mats[m] + 6 * i;
						std::fprintf(f, "  [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g],\n", row[0], row[1], row[2], row[3], row[4], row[5]);
					}
					std::fprintf(f, "]\n");
				}
				std::fclose(f);
			}
		}
		if (!config.io.visualization.empty()) engine.write_visualization(config.io.visualization);
		for (size_t k = 0; k < source_list.size(); k++) {
			// the next scan on the same engine: only the source stage of creation is redone
			std::vector<P3> next;
			load_cloud(source_list[k], config.subsample, config.resize, next, seed);
			const auto t0 = std::chrono::steady_clock::now();
			size_t kept = next.size();
			if (plane_sel[0].distance > 0.f) {
				goicp_source_pipeline sp;
				goicp_source_pipeline_default(&sp);
				sp.voxel = voxel; sp.stat_neighbors = stat_k[0]; sp.stat_std_ratio = stat_ratio[0];
				sp.radius = outlier_radius[0]; sp.min_neighbors = outlier_min[0];
				kept = engine.set_source(next, &sp, plane_sel[0], cluster[0].radius > 0.f ? &cluster[0] : nullptr);
				std::printf("source %zu plane distance %g iterations %d max %d min inliers %d refine %d: kept %zu of %zu points\n", k + 1, plane_sel[0].distance,
				            (int)plane_sel[0].iterations, (int)plane_sel[0].max_planes, (int)plane_sel[0].min_inliers, (int)plane_sel[0].refine, kept, next.size());
			} else if (cluster[0].radius > 0.f) {
				goicp_source_pipeline sp;
				goicp_source_pipeline_default(&sp);
				sp.voxel = voxel; sp.stat_neighbors = stat_k[0]; sp.stat_std_ratio = stat_ratio[0];
				sp.radius = outlier_radius[0]; sp.min_neighbors = outlier_min[0];
				kept = engine.set_source(next, &sp, cluster[0]);
				std::printf("source %zu cluster radius %g min neighbors %d min size %d keep %d: kept %zu of %zu points\n", k + 1, cluster[0].radius,
				            (int)cluster[0].min_neighbors, (int)cluster[0].min_size, (int)cluster[0].max_clusters, kept, next.size());
			} else if (stat_k[0] > 0) {
				goicp_source_pipeline sp;
				goicp_source_pipeline_default(&sp);
				sp.voxel = voxel; sp.stat_neighbors = stat_k[0]; sp.stat_std_ratio = stat_ratio[0];
				sp.radius = outlier_radius[0]; sp.min_neighbors = outlier_min[0];
				kept = engine.set_source(next, sp);
				std::printf("source %zu stat neighbors %d std ratio %g: kept %zu of %zu points\n", k + 1, sp.stat_neighbors, sp.stat_std_ratio, kept, next.size());
			} else if (outlier_radius[0] > 0.f) {
				goicp_source_filter f;
				goicp_source_filter_default(&f);
				f.voxel = voxel; f.radius = outlier_radius[0]; f.min_neighbors = outlier_min[0];
				kept = engine.set_source(next, f);
				std::printf("source %zu outlier radius %g min neighbors %d: kept %zu of %zu points\n", k + 1, f.radius, f.min_neighbors, kept, next.size());
			} else if (voxel > 0.f) kept = engine.set_source(next, voxel); else engine.set_source(next);
			const double swap_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
			if (config.mode <= 2) {
				for (int i = 0; i < iters; i++) check(goicp_icp_step(h));
			} else {
				engine.run();
			}
			check(goicp_poll(h, &r));
			std::printf("source %zu (%s): %zu points, swap %.3f ms, register %.1f ms, Best Error: %.7g, rotation nodes %lld\n", k + 1, source_list[k].c_str(), kept,
			            swap_ms, r.register_ms, r.best_sse, (long long)r.counters.rot_pops);
			if (!config.io.output.empty()) engine.write_output(numbered(config.io.output, (int)k + 1));
			if (!config.io.visualization.empty()) engine.write_visualization(numbered(config.io.visualization, (int)k + 1));
		}
	} catch (const std::exception& e) {
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
	return 0;
}
