// goicp_mi355.hpp -- header-only C++ shim over the C ABI (goicp_mi355.h) that re-creates the reference's class
// and step-function surface, so that the reference's own call sites compile against this engine:
//     Config / load_cloud                               src/common.h:133-180, src/common.cpp:205-228
//     icp::RotNode / TransNode / StreamPool             src/fgoicp/fgoicp_common.hpp:64-167
//     icp::Registration::compute_sse_error x2           src/fgoicp/registration.hpp:96-97
//     icp::IterativeClosestPoint3D::run                 src/fgoicp/icp3d.hpp:30-35
//     icp::FastGoICP{run,get_best_error,optR,optT,curR,curT,finished}   src/fgoicp/fgoicp.hpp:11-69  (ctor: src/main.cpp:94,
//                                                       worker: src/main.cpp:150)
//     PointCloud::initBuffers / cleanupBuffers          src/kernel.h:57-61
//     ICP::naiveGPUStep / kdTreeGPUStep / CPUStep       src/icp_kernel.h:9-13
//     ICP::goicpGPUStep                                 src/goicp_kernel.h:6-10, src/goicp_kernel.cu:161-177
//
// Matrix / vector types.  The reference uses glm::mat3 / glm::vec3.  When glm is visible (any glm header was included
// before this one, or GOICP_MI355_USE_GLM is defined) Mat3 / Vec3 ARE glm::mat3 / glm::vec3, so reference statements such
// as `prev_optR != fgoicp->optR` or `prev_optR = fgoicp->optR` compile unchanged.  Without glm the shim supplies
// layout-compatible stand-ins (column-major 3x3, `m[col][row]`, like glm).  The C ABI underneath is row-major float[9];
// the conversion happens here.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#if defined(GOICP_MI355_USE_GLM) && !defined(GLM_VERSION)
#include <glm/mat3x3.hpp>
#include <glm/vec3.hpp>
#endif

#include "goicp_mi355.h"

namespace goicp_mi355 {

#if defined(GLM_VERSION)
using Mat3 = glm::mat3;
using Vec3 = glm::vec3;
#else
struct Vec3 {
	float x = 0.f, y = 0.f, z = 0.f;
	Vec3() = default;
	explicit Vec3(float s) : x(s), y(s), z(s) {}
	Vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
	float& operator[](int i) { return (&x)[i]; }
	const float& operator[](int i) const { return (&x)[i]; }
	friend bool operator==(const Vec3& a, const Vec3& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
	friend bool operator!=(const Vec3& a, const Vec3& b) { return !(a == b); }
};
struct Mat3 {            // column-major like glm::mat3: m[col][row]
	Vec3 c[3];
	Mat3() : Mat3(1.0f) {}
	explicit Mat3(float d) { c[0] = Vec3(d, 0, 0); c[1] = Vec3(0, d, 0); c[2] = Vec3(0, 0, d); }
	Vec3& operator[](int i) { return c[i]; }
	const Vec3& operator[](int i) const { return c[i]; }
	friend bool operator==(const Mat3& a, const Mat3& b) { return a.c[0] == b.c[0] && a.c[1] == b.c[1] && a.c[2] == b.c[2]; }
	friend bool operator!=(const Mat3& a, const Mat3& b) { return !(a == b); }
};
#endif
static_assert(sizeof(Vec3) == 3 * sizeof(float) && sizeof(Mat3) == 9 * sizeof(float), "packed float vector / matrix types expected");

// row-major float[9] (C ABI) <-> column-major Mat3
inline void to_rows(const Mat3& M, float r[9])
{
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) r[3 * i + j] = M[j][i];
}
inline Mat3 from_rows(const float r[9])
{
	Mat3 M(1.0f);
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) M[j][i] = r[3 * i + j];
	return M;
}
inline Vec3 from_xyz(const float t[3]) { return Vec3(t[0], t[1], t[2]); }

inline void check(int status)
{
	if (status != GOICP_OK) throw std::runtime_error(goicp_last_error());   // the reference throws std::runtime_error too
}

// class Config (src/common.h:133-180): same public fields
class Config {
public:
	int mode = 1;
	bool trim = false;
	float subsample = 1.0f, mse_threshold = 1e-5f, resize = 1.0f;
	struct IO { std::string target, source, output, visualization; } io;
	struct Viz { float phi = 0.4f, theta = 0.0f; bool spin_after_finish = false; } viz;
	struct Range { float xmin, xmax, ymin, ymax, zmin, zmax; int search_depth; } rotation{}, translation{};
	goicp_config raw{};     // the parsed C struct (goicp_params_from_config(&config.raw, &params) hands the ranges to the engine)

	explicit Config(const std::string toml_filepath)
	{
		goicp_config& c = raw;
		check(goicp_config_load(toml_filepath.c_str(), &c));
		mode = c.mode; trim = c.trim != 0; subsample = c.subsample; mse_threshold = c.mse_threshold; resize = c.resize;
		io = {c.target, c.source, c.output, c.visualization};
		viz.phi = c.viz_phi; viz.theta = c.viz_theta; viz.spin_after_finish = c.viz_spin_after_finish != 0;
		rotation = {c.rot_min[0], c.rot_max[0], c.rot_min[1], c.rot_max[1], c.rot_min[2], c.rot_max[2], c.rot_search_depth};
		translation = {c.trans_min[0], c.trans_max[0], c.trans_min[1], c.trans_max[1], c.trans_min[2], c.trans_max[2], c.trans_search_depth};
	}
};

// size_t load_cloud(path, subsample, resize, cloud) (src/common.cpp:205-228): appends to `cloud`
template <class Point3>
size_t load_cloud(const std::string& filepath, const float& subsample, const float& resize, std::vector<Point3>& cloud,
                  uint64_t seed = 0)
{
	static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats (e.g. glm::vec3)");
	float* xyz = nullptr;
	size_t n = 0;
	check(goicp_cloud_load(filepath.c_str(), subsample, resize, seed, &xyz, &n));
	const Point3* p = reinterpret_cast<const Point3*>(xyz);
	cloud.insert(cloud.end(), p, p + n);
	goicp_cloud_free(xyz);
	return n;
}

namespace icp {

// src/fgoicp/fgoicp_common.hpp:139-167.  The engine owns its HIP stream; the pool only keeps call sites compiling.
class StreamPool {
public:
	explicit StreamPool(size_t size) : size_(size) {}
	size_t size() const { return size_; }
private:
	size_t size_;
};

// Rotation cube (src/fgoicp/fgoicp_common.hpp:31-104) with the CPU path's parametrisation, which is the one the
// engine implements (src/goicp/jly_goicp.h:44-57, jly_goicp.cpp:433-467): (x,y,z) = the cube CENTRE as an angle-axis
// vector (radians), span = half edge length, R = its Rodrigues matrix.
struct Rotation {
	float x, y, z, r;
	Mat3 R;
	Rotation() : Rotation(0.f, 0.f, 0.f) {}
	Rotation(float x_, float y_, float z_) : x(x_), y(y_), z(z_), r(std::sqrt(x_ * x_ + y_ * y_ + z_ * z_)), R(1.0f)
	{
		const float v[3] = {x, y, z};
		float rows[9];
		goicp_rodrigues(v, rows);
		R = from_rows(rows);
	}
	bool in_SO3() const { return r <= 3.14159265358979f; }
};
struct RotNode {
	Rotation q;
	float span;
	float lb, ub;
	RotNode(float x, float y, float z, float span_, float lb_, float ub_) : q(x, y, z), span(span_), lb(lb_), ub(ub_) {}
	friend bool operator<(const RotNode& a, const RotNode& b) { return a.lb == b.lb ? a.span < b.span : a.lb > b.lb; }
	// pi-ball test of GoICP::OuterBnB (src/goicp/jly_goicp.cpp:443)
	bool overlaps_SO3() const { return (double)q.r - 1.732050808 * (double)(2 * span) / 2 <= 3.1415926536; }
	// level l <=> cube width 2*pi / 2^l (src/goicp/jly_goicp.cpp:148-160: one radius table per level)
	int level() const
	{
		const double l = std::log2(3.1415926536 / (double)span);
		return l <= 0 ? 0 : (int)(l + 0.5);
	}
};
struct TransNode {            // centre + half-width (src/fgoicp/fgoicp_common.hpp:108-129)
	Vec3 t;
	float span;
	float lb, ub;
	TransNode(float x, float y, float z, float span_, float lb_, float ub_) : t(x, y, z), span(span_), lb(lb_), ub(ub_) {}
	friend bool operator<(const TransNode& a, const TransNode& b) { return a.lb == b.lb ? a.span < b.span : a.lb > b.lb; }
};

class Registration {
public:
	template <class Point3>
	Registration(const std::vector<Point3>& pct, size_t nt, const std::vector<Point3>& pcs, size_t ns, float mse_threshold = 1e-3f,
	             const goicp_params* params = nullptr)
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		goicp_params p;
		if (params) p = *params; else goicp_params_default(&p);
		p.mse_threshold = mse_threshold;
		check(goicp_create(&p, reinterpret_cast<const float*>(pct.data()), nt, reinterpret_cast<const float*>(pcs.data()), ns, &h_));
		ns_ = ns;
	}
	~Registration() { goicp_destroy(h_); }
	Registration(const Registration&) = delete;
	Registration& operator=(const Registration&) = delete;

	using BoundsResult_t = std::tuple<std::vector<float>, std::vector<float>>;   // (lb, ub) as the reference

	// float compute_sse_error(glm::mat3 R, glm::vec3 t) const        (registration.hpp:96)
	float compute_sse_error(Mat3 R, Vec3 t) const
	{
		float rows[9], tt[3] = {t[0], t[1], t[2]}, sse = 0.f;
		to_rows(R, rows);
		check(goicp_eval_sse(h_, rows, tt, &sse));
		return sse;
	}
	// BoundsResult_t compute_sse_error(RotNode&, std::vector<TransNode>&, bool fix_rot, StreamPool&) const   (registration.hpp:97)
	BoundsResult_t compute_sse_error(RotNode& rnode, std::vector<TransNode>& tnodes, bool fix_rot, StreamPool&) const
	{
		return bounds(rnode.q.R, fix_rot ? -1 : rnode.level(), tnodes);
	}
	// the same with an explicit rotation level (rot_level < 0 <=> fix_rot)
	BoundsResult_t compute_sse_error(const Mat3& R, int rot_level, const std::vector<TransNode>& tnodes) const { return bounds(R, rot_level, tnodes); }
	goicp_handle handle() const { return h_; }
	// a new source cloud under the same target (goicp_set_source): everything built from the target, the params and the options set on this
	// registration stay; afterwards it answers as one constructed with (pct, pcs) and the same options would
	template <class Point3>
	void set_source(const std::vector<Point3>& pcs, size_t ns)
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		check(goicp_set_source(h_, reinterpret_cast<const float*>(pcs.data()), ns));
		ns_ = ns;
	}
	// the same behind a voxel grid (goicp_set_source_voxel): the cloud is reduced to one centroid per occupied cell of pitch `voxel` on the
	// device, then swapped in; returns the number of points kept, which is the registration's source size from here on
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, size_t ns, float voxel)
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		size_t kept = 0;
		check(goicp_set_source_voxel(h_, reinterpret_cast<const float*>(pcs.data()), ns, voxel, &kept));
		ns_ = kept;
		return kept;
	}
	// the same behind the whole filter chain (goicp_set_source_filtered): the voxel grid when f.voxel > 0, then radius outlier removal when
	// f.radius > 0 (points with fewer than f.min_neighbors others within f.radius are dropped), all on the device; returns the points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, size_t ns, const goicp_source_filter& f)
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		size_t kept = 0;
		check(goicp_set_source_filtered(h_, reinterpret_cast<const float*>(pcs.data()), ns, &f, &kept));
		ns_ = kept;
		return kept;
	}
	// the same behind the three-stage chain (goicp_set_source_pipeline): the voxel grid when p.voxel > 0, then statistical outlier removal
	// when p.stat_neighbors > 0 (mean distance to the nearest neighbours above the mean plus p.stat_std_ratio deviations), then radius
	// outlier removal when p.radius > 0, all on the device; returns the points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, size_t ns, const goicp_source_pipeline& p)
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		size_t kept = 0;
		check(goicp_set_source_pipeline(h_, reinterpret_cast<const float*>(pcs.data()), ns, &p, &kept));
		ns_ = kept;
		return kept;
	}
	// the same behind the pipeline's stages and the cluster selection (goicp_set_source_clustered): after p's stages (p may be null), only the
	// points of the s.max_clusters largest clusters (0 = all) with at least s.min_size members stay; returns the points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, size_t ns, const goicp_source_pipeline* p, const goicp_cluster_select& s)
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		size_t kept = 0;
		check(goicp_set_source_clustered(h_, reinterpret_cast<const float*>(pcs.data()), ns, p, &s, &kept));
		ns_ = kept;
		return kept;
	}
	// Euclidean / DBSCAN clustering of any cloud, on the device (goicp_cluster): label gets n entries (-1 = noise), sizes the c clusters'
	// sizes; returns c.  The registration lends its device, its state is untouched
	template <class Point3>
	size_t cluster(const std::vector<Point3>& cloud, size_t n, float radius, int min_neighbors, std::vector<int32_t>& label, std::vector<int32_t>* sizes = nullptr) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		label.resize(n);
		if (sizes) sizes->resize(n);
		size_t c = 0;
		check(goicp_cluster(h_, reinterpret_cast<const float*>(cloud.data()), n, radius, (int32_t)min_neighbors, label.data(), sizes ? sizes->data() : nullptr, &c));
		if (sizes) sizes->resize(c);
		return c;
	}
	// the points of the selected clusters of any cloud, on the device (goicp_cluster_filter), in input order: kept gets the m points, index
	// and label (each may be null) their original indices and cluster labels; returns m
	template <class Point3>
	size_t cluster_filter(const std::vector<Point3>& cloud, size_t n, const goicp_cluster_select& s, std::vector<Point3>& kept,
	                      std::vector<int32_t>* index = nullptr, std::vector<int32_t>* label = nullptr) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		kept.resize(n);
		if (index) index->resize(n);
		if (label) label->resize(n);
		size_t m = 0;
		check(goicp_cluster_filter(h_, reinterpret_cast<const float*>(cloud.data()), n, &s, reinterpret_cast<float*>(kept.data()), index ? index->data() : nullptr,
		                           label ? label->data() : nullptr, &m));
		kept.resize(m);
		if (index) index->resize(m);
		if (label) label->resize(m);
		return m;
	}
	// the full chain (goicp_set_source_segmented): after p's stages (p may be null) the points of the planes `pl` finds are dropped, then the
	// cluster selection s (may be null) runs; returns the points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, size_t ns, const goicp_source_pipeline* p, const goicp_plane_select& pl, const goicp_cluster_select* s)
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		size_t kept = 0;
		check(goicp_set_source_segmented(h_, reinterpret_cast<const float*>(pcs.data()), ns, p, &pl, s, &kept));
		ns_ = kept;
		return kept;
	}
	// RANSAC plane segmentation of any cloud, on the device (goicp_segment_plane): label gets n entries (-1 = no plane), planes the planes
	// found; returns their number.  The registration lends its device, its state is untouched
	template <class Point3>
	size_t segment_plane(const std::vector<Point3>& cloud, size_t n, const goicp_plane_select& sel, std::vector<int32_t>& label, std::vector<goicp_plane>& planes) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		label.resize(n);
		planes.resize(GOICP_PLANE_MAX_PLANES);
		size_t c = 0;
		check(goicp_segment_plane(h_, reinterpret_cast<const float*>(cloud.data()), n, &sel, label.data(), planes.data(), &c));
		planes.resize(c);
		return c;
	}
	// the points no plane took, on the device (goicp_plane_filter), in input order: kept gets the m points, index and planes (each may be
	// null) their original indices and the planes found; returns m
	template <class Point3>
	size_t plane_filter(const std::vector<Point3>& cloud, size_t n, const goicp_plane_select& sel, std::vector<Point3>& kept, std::vector<int32_t>* index = nullptr,
	                    std::vector<goicp_plane>* planes = nullptr) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		kept.resize(n);
		if (index) index->resize(n);
		if (planes) planes->resize(GOICP_PLANE_MAX_PLANES);
		size_t m = 0, c = 0;
		check(goicp_plane_filter(h_, reinterpret_cast<const float*>(cloud.data()), n, &sel, reinterpret_cast<float*>(kept.data()), index ? index->data() : nullptr,
		                         planes ? planes->data() : nullptr, &c, &m));
		kept.resize(m);
		if (index) index->resize(m);
		if (planes) planes->resize(c);
		return m;
	}
	// the exact k nearest other points of every point of any cloud, on the device (goicp_knn_self): index gets n x k entries, row i ascending
	// by (squared distance, index); dist_sq (may be null) their squared distances.  The registration lends its device, its state is untouched
	template <class Point3>
	void knn_self(const std::vector<Point3>& cloud, size_t n, int k, std::vector<int32_t>& index, std::vector<float>* dist_sq = nullptr) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		index.resize(k > 0 ? n * (size_t)k : 0);
		if (dist_sq) dist_sq->resize(index.size());
		check(goicp_knn_self(h_, reinterpret_cast<const float*>(cloud.data()), n, (int32_t)k, index.data(), dist_sq ? dist_sq->data() : nullptr));
	}
	// per-point normals of any cloud, on the device (goicp_estimate_normals): the k-point neighbourhood counts the point itself; viewpoint (may
	// be null) flips every normal towards it; variation (may be null) gets the surface variation (PCL's curvature) of every point
	template <class Point3>
	void estimate_normals(const std::vector<Point3>& cloud, size_t n, int k, const float* viewpoint, std::vector<Point3>& normals,
	                      std::vector<float>* variation = nullptr) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		normals.resize(n);
		if (variation) variation->resize(n);
		check(goicp_estimate_normals(h_, reinterpret_cast<const float*>(cloud.data()), n, (int32_t)k, viewpoint, reinterpret_cast<float*>(normals.data()),
		                             variation ? variation->data() : nullptr, nullptr));
	}
	// the 33-bin FPFH descriptor of every point of any cloud with its normals, on the device (goicp_fpfh): descriptors gets n x GOICP_FPFH_DIM
	// floats; k counts the nearest other points; spfh_counts (may be null) gets the n x GOICP_FPFH_DIM counts of the simplified histograms
	template <class Point3>
	void fpfh(const std::vector<Point3>& cloud, const std::vector<Point3>& normals, size_t n, int k, std::vector<float>& descriptors,
	          std::vector<uint8_t>* spfh_counts = nullptr) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		if (normals.size() < n || cloud.size() < n) throw std::runtime_error("fpfh: one point and one normal per descriptor");
		descriptors.resize(n * (size_t)GOICP_FPFH_DIM);
		if (spfh_counts) spfh_counts->resize(descriptors.size());
		check(goicp_fpfh(h_, reinterpret_cast<const float*>(cloud.data()), reinterpret_cast<const float*>(normals.data()), n, (int32_t)k, descriptors.data(),
		                 spfh_counts ? spfh_counts->data() : nullptr));
	}
	// the nearest target descriptor of every query descriptor, on the device (goicp_match_features; n_q * n_t pairs: for downsampled clouds).
	// index, d2 and d2_second get one entry per query; mutual (may be null) 1 where the match holds in both directions
	void match_features(const std::vector<float>& query, const std::vector<float>& target, std::vector<int32_t>& index, std::vector<float>& d2,
	                    std::vector<float>& d2_second, std::vector<uint8_t>* mutual = nullptr) const
	{
		const size_t nq = query.size() / GOICP_FPFH_DIM, nt = target.size() / GOICP_FPFH_DIM;
		index.resize(nq); d2.resize(nq); d2_second.resize(nq);
		if (mutual) mutual->resize(nq);
		check(goicp_match_features(h_, query.data(), nq, target.data(), nt, index.data(), d2.data(), d2_second.data(), mutual ? mutual->data() : nullptr));
	}
	// match_features' output as correspondences (goicp_select_matches, host only): corr gets the M kept pairs (query, target) flat, 2 M ints;
	// mutual may be null when require_mutual is false; ratio 0 = no ratio test; returns M
	static size_t select_matches(const std::vector<int32_t>& index, const std::vector<float>& d2, const std::vector<float>& d2_second,
	                             const std::vector<uint8_t>* mutual, float ratio, bool require_mutual, std::vector<int32_t>& corr)
	{
		const size_t nq = index.size();
		if (d2.size() != nq || d2_second.size() != nq || (mutual && mutual->size() != nq)) throw std::invalid_argument("select_matches: one entry per query");
		corr.resize(2 * nq);
		size_t m = 0;
		check(goicp_select_matches(index.data(), d2.data(), d2_second.data(), mutual ? mutual->data() : nullptr, nq, ratio, require_mutual ? 1 : 0, corr.data(), &m));
		corr.resize(2 * m);
		return m;
	}
	// RANSAC pose estimation from correspondences, on the device (goicp_ransac_pose): corr holds M pairs (source index, target index) flat;
	// poses gets the poses found (at most sel.max_poses), inlier (may be null) the M verdicts under poses[0]; returns the number of poses
	template <class Point3>
	size_t ransac_pose(const std::vector<Point3>& src, const std::vector<Point3>& tgt, const std::vector<int32_t>& corr, const goicp_ransac_pose_select& sel,
	                   std::vector<goicp_ransac_pose_result>& poses, std::vector<uint8_t>* inlier = nullptr) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		const size_t M = corr.size() / 2;
		poses.resize(GOICP_RANSAC_POSE_MAX_POSES);
		if (inlier) inlier->resize(M);
		size_t c = 0;
		check(goicp_ransac_pose(h_, reinterpret_cast<const float*>(src.data()), src.size(), reinterpret_cast<const float*>(tgt.data()), tgt.size(), corr.data(), M, &sel,
		                        poses.data(), &c, inlier ? inlier->data() : nullptr));
		poses.resize(c);
		return c;
	}
	// the metric of every ICP this registration runs (goicp_set_icp_options): 0 point-to-point (default), 1 point-to-plane
	void set_icp_options(int metric, int normal_k = 16)
	{
		goicp_icp_options o{metric, normal_k};
		check(goicp_set_icp_options(h_, &o));
	}
	// metric 1 in its symmetric form over the normals of both clouds (goicp_set_icp_symmetric); stored and inert under metric 0
	void set_icp_symmetric(bool enabled, int source_normal_k = 16) { check(goicp_set_icp_symmetric(h_, enabled ? 1 : 0, (int32_t)source_normal_k)); }
	struct IcpSymmetric { bool enabled; int source_normal_k; bool user_normals; };
	IcpSymmetric icp_symmetric() const
	{
		int32_t e = 0, k = 0, u = 0;
		check(goicp_get_icp_symmetric(h_, &e, &k, &u));
		return IcpSymmetric{e != 0, (int)k, u != 0};
	}
	// metric 1 in its generalized (plane-to-plane) form, each correspondence weighted by the combined covariance of both clouds' normals
	// (goicp_set_icp_generalized); stored and inert under metric 0; the symmetric flag and this one refuse each other
	void set_icp_generalized(bool enabled, float epsilon = 1e-3f, int source_normal_k = 16)
	{
		check(goicp_set_icp_generalized(h_, enabled ? 1 : 0, epsilon, (int32_t)source_normal_k));
	}
	struct IcpGeneralized { bool enabled; float epsilon; int source_normal_k; bool user_normals; };
	IcpGeneralized get_icp_generalized() const
	{
		int32_t e = 0, k = 0, u = 0;
		float eps = 0.f;
		check(goicp_get_icp_generalized(h_, &e, &eps, &k, &u));
		return IcpGeneralized{e != 0, eps, (int)k, u != 0};
	}
	// the source normals the symmetric and the generalized form read (original source order): the estimated ones, built on first use, or the caller's
	template <class Point3>
	void source_normals(std::vector<Point3>& normals) const
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		normals.resize(ns_);
		check(goicp_source_normals(h_, reinterpret_cast<float*>(normals.data())));
	}
	// the caller's own normals (each zero or of unit length) until the next source swap (goicp_set_source_normals)
	template <class Point3>
	void set_source_normals(const std::vector<Point3>& normals)
	{
		static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
		check(goicp_set_source_normals(h_, reinterpret_cast<const float*>(normals.data()), normals.size()));
	}
	// a maximum correspondence distance for every ICP this registration runs (goicp_set_icp_gate); 0 switches it off
	void set_icp_gate(float max_corr_dist, int min_inliers = 0, int capped_walk = 1)
	{
		goicp_icp_gate g{max_corr_dist, min_inliers, capped_walk};
		check(goicp_set_icp_gate(h_, &g));
	}
	// a robust kernel for every ICP this registration runs (goicp_set_icp_robust): 1 Huber, 2 Cauchy, 3 Geman-McClure, 4 Tukey; 0 switches it off
	void set_icp_robust(int kernel, float scale = 0.f)
	{
		goicp_icp_robust r{kernel, scale};
		check(goicp_set_icp_robust(h_, &r));
	}
	// the objective of the SEARCH (goicp_set_search_truncation): bounds, pose scores and best_sse become sum min(DT(R p + t), max_dist)^2; 0 switches it off
	void set_search_truncation(float max_dist) { check(goicp_set_search_truncation(h_, max_dist)); }
	// goicp_pose_information at R | t: information matrix, gradient, covariance, eigen-decomposition and rank (the struct is the C ABI's plain
	// goicp_pose_info); opt = nullptr: the handle's metric, the transformed source centroid as pivot, the default rank_tol
	goicp_pose_info pose_information(const float R[9], const float t[3], const goicp_pose_info_options* opt = nullptr)
	{
		goicp_pose_info out;
		check(goicp_pose_information(h_, R, t, opt, &out));
		return out;
	}
	float search_truncation() const
	{
		float g = 0.f;
		check(goicp_search_truncation(h_, &g));
		return g;
	}
	// goicp_eval_correspondences at R|t: neighbour index per source point (-1 beyond the gate) and squared distance; returns the inlier count
	int eval_correspondences(Mat3 R, Vec3 t, float max_corr_dist, std::vector<int32_t>* index = nullptr, std::vector<float>* dist_sq = nullptr,
	                         float* sse_inliers = nullptr) const
	{
		float rows[9], tt[3] = {t[0], t[1], t[2]};
		to_rows(R, rows);
		int32_t n = 0;
		std::vector<int32_t> idx;
		std::vector<float> d2;
		if (index) idx.resize(ns_);
		if (dist_sq) d2.resize(ns_);
		check(goicp_eval_correspondences(h_, rows, tt, max_corr_dist, index ? idx.data() : nullptr, dist_sq ? d2.data() : nullptr, &n, sse_inliers));
		if (index) *index = idx;
		if (dist_sq) *dist_sq = d2;
		return (int)n;
	}

private:
	BoundsResult_t bounds(const Mat3& R, int rot_level, const std::vector<TransNode>& tnodes) const
	{
		std::vector<float> cubes(4 * tnodes.size()), lb(tnodes.size()), ub(tnodes.size());
		for (size_t i = 0; i < tnodes.size(); i++) {
			cubes[4 * i] = tnodes[i].t[0]; cubes[4 * i + 1] = tnodes[i].t[1]; cubes[4 * i + 2] = tnodes[i].t[2];
			cubes[4 * i + 3] = 2 * tnodes[i].span;
		}
		float rows[9];
		to_rows(R, rows);
		check(goicp_eval_bounds(h_, rows, cubes.data(), tnodes.size(), rot_level, ub.data(), lb.data()));
		return {lb, ub};
	}
	goicp_handle h_ = nullptr;
	size_t ns_ = 0;
};

class IterativeClosestPoint3D {
public:
	IterativeClosestPoint3D(const Registration& reg, size_t max_iter, float convergence_threshold, Mat3 R, Vec3 t)
	    : reg_(reg), max_iter_(max_iter), thr_(convergence_threshold), R_(R), t_(t) {}
	// the reference's argument list (icp3d.hpp:30): the clouds already live in `reg`
	template <class PointCloud>
	IterativeClosestPoint3D(const Registration& reg, const PointCloud&, const PointCloud&, size_t max_iter, float convergence_threshold, Mat3 R, Vec3 t)
	    : IterativeClosestPoint3D(reg, max_iter, convergence_threshold, R, t) {}
	using Result_t = std::tuple<float, Mat3, Vec3>;
	Result_t run(Mat3& curR, Vec3& curT)
	{
		float err = 0.f, rows[9], tt[3] = {t_[0], t_[1], t_[2]};
		int32_t it = 0;
		to_rows(R_, rows);
		check(goicp_icp_run(reg_.handle(), rows, tt, (int32_t)max_iter_, thr_, &err, &it));
		R_ = from_rows(rows); t_ = from_xyz(tt);
		curR = R_; curT = t_;
		return Result_t{err, R_, t_};
	}
	// multi-start form (goicp_icp_run_batch): refines every pose of R / t (same length, at most 1024) in place with this object's
	// max_iter and threshold; pose k ends as run() from R[k], t[k] would leave it.  Returns each pose's error; iters (optional) its iterations
	std::vector<float> run_batch(std::vector<Mat3>& R, std::vector<Vec3>& t, std::vector<int32_t>* iters = nullptr) const
	{
		if (R.size() != t.size()) throw std::invalid_argument("IterativeClosestPoint3D::run_batch: R and t differ in length");
		const size_t K = R.size();
		std::vector<float> rows(9 * K), tt(3 * K), err(K);
		std::vector<int32_t> it(K);
		for (size_t k = 0; k < K; k++) {
			to_rows(R[k], &rows[9 * k]);
			for (int i = 0; i < 3; i++) tt[3 * k + i] = t[k][i];
		}
		check(goicp_icp_run_batch(reg_.handle(), K, rows.data(), tt.data(), (int32_t)max_iter_, thr_, err.data(), it.data()));
		for (size_t k = 0; k < K; k++) { R[k] = from_rows(&rows[9 * k]); t[k] = from_xyz(&tt[3 * k]); }
		if (iters) *iters = it;
		return err;
	}

private:
	const Registration& reg_;
	size_t max_iter_;
	float thr_;
	Mat3 R_;
	Vec3 t_;
};

// icp::FastGoICP (src/fgoicp/fgoicp.hpp:11-69).  As in the reference the worker thread (run()) keeps the public
// members optR / optT / curR / curT / finished current and the reader locks `mtx` while it reads them
// (src/goicp_kernel.cu:164-177) -- here the writes happen under the same mutex (goicp_set_progress_callback), which
// the reference forgot (src/fgoicp/fgoicp.cpp:68-69,85-86).
class FastGoICP {
public:
	template <class Point3>
	FastGoICP(std::vector<Point3>& pct, std::vector<Point3>& pcs, float mse_threshold, std::mutex& mtx_,
	          const goicp_params* params = nullptr)
	    : curR(1.0f), optR(1.0f), curT(0.0f), optT(0.0f), finished(false), mtx(mtx_),
	      registration(pct, pct.size(), pcs, pcs.size(), mse_threshold, params)
	{
		check(goicp_set_progress_callback(registration.handle(), &FastGoICP::on_progress, this));
		sync();
	}
	~FastGoICP() { goicp_set_progress_callback(registration.handle(), nullptr, nullptr); }
	FastGoICP(const FastGoICP&) = delete;

	void run()
	{
		check(goicp_register(registration.handle()));
		sync();
	}
	// Registration::set_source, then the public members are the fresh handle's (identity poses, not finished)
	template <class Point3>
	void set_source(const std::vector<Point3>& pcs)
	{
		registration.set_source(pcs, pcs.size());
		sync();
	}
	// ... behind a voxel grid of pitch `voxel`; returns the number of points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, float voxel)
	{
		const size_t kept = registration.set_source(pcs, pcs.size(), voxel);
		sync();
		return kept;
	}
	// ... behind the filter chain `f` (voxel grid, then radius outlier removal); returns the number of points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, const goicp_source_filter& f)
	{
		const size_t kept = registration.set_source(pcs, pcs.size(), f);
		sync();
		return kept;
	}
	// ... behind the three-stage chain `p` (voxel grid, statistical outlier removal, radius outlier removal); returns the number of points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, const goicp_source_pipeline& p)
	{
		const size_t kept = registration.set_source(pcs, pcs.size(), p);
		sync();
		return kept;
	}
	// ... behind the chain `p` (may be null) and the cluster selection `s` (keep the largest clusters); returns the number of points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, const goicp_source_pipeline* p, const goicp_cluster_select& s)
	{
		const size_t kept = registration.set_source(pcs, pcs.size(), p, s);
		sync();
		return kept;
	}
	// ... behind the chain `p` (may be null), the plane removal `pl` and the cluster selection `s` (may be null); returns the number of points kept
	template <class Point3>
	size_t set_source(const std::vector<Point3>& pcs, const goicp_source_pipeline* p, const goicp_plane_select& pl, const goicp_cluster_select* s)
	{
		const size_t kept = registration.set_source(pcs, pcs.size(), p, pl, s);
		sync();
		return kept;
	}
	void cancel() { goicp_cancel(registration.handle()); }
	float get_best_error() const { return best_sse; }       // fgoicp.hpp:34; read under `mtx` like the other members
	void sync()
	{
		goicp_result r;
		check(goicp_poll(registration.handle(), &r));
		std::lock_guard<std::mutex> lk(mtx);
		take(r);
	}
	// goicp_result_information: the same at optR | optT of the last finished registration
	goicp_pose_info information(const goicp_pose_info_options* opt = nullptr)
	{
		goicp_pose_info out;
		check(goicp_result_information(registration.handle(), opt, &out));
		return out;
	}
	void write_output(const std::string& path) { check(goicp_result_write_toml(registration.handle(), path.c_str())); }
	void write_visualization(const std::string& path) { check(goicp_result_write_ply(registration.handle(), path.c_str())); }

	// For visualization (fgoicp.hpp:66-69)
	Mat3 curR, optR;
	Vec3 curT, optT;
	bool finished;

private:
	static void on_progress(const goicp_result* r, void* self)
	{
		FastGoICP* f = static_cast<FastGoICP*>(self);
		std::lock_guard<std::mutex> lk(f->mtx);
		f->take(*r);
	}
	void take(const goicp_result& r)
	{
		optR = from_rows(r.optR); curR = from_rows(r.curR);
		optT = from_xyz(r.optT); curT = from_xyz(r.curT);
		best_sse = r.best_sse;
		finished = r.finished != 0;
	}
	float best_sse = 1e10f;
	std::mutex& mtx;

public:
	Registration registration;
};

}  // namespace icp

// ------------------------------------------------------------------------------------------------------------------
// Step API (src/icp_kernel.h:9-13, src/goicp_kernel.h:6-10).  The reference's step functions work on global device
// buffers set up by PointCloud::initBuffers(Ybuffer = data, Xbuffer = model) (src/kernel.cu:60-110) and publish the
// moved cloud to the viewer; here the "global buffers" are one engine instance, and the moved source cloud is
// available from step_positions().  All arithmetic runs in the HIP library -- also for ICP::CPUStep, whose host
// vectors are updated from the device result (this engine has no CPU compute path).
// ------------------------------------------------------------------------------------------------------------------
struct StepGlobals {
	std::unique_ptr<icp::Registration> reg;
	size_t numDataPoints = 0, numModelPoints = 0;
	bool goicp_finished = false;       // the reference's global flag (src/main.cpp:27, goicp_kernel.cu:167)
	float sse_threshold = 0.f;         // src/main.cpp:42
};
inline StepGlobals& step_globals()
{
	static StepGlobals g;
	return g;
}

namespace PointCloud {
template <class Point3>
inline void initBuffers(std::vector<Point3>& Ybuffer, std::vector<Point3>& Xbuffer, const goicp_params* params = nullptr)
{
	StepGlobals& g = step_globals();
	g.reg.reset(new icp::Registration(Xbuffer, Xbuffer.size(), Ybuffer, Ybuffer.size(), 1e-3f, params));
	g.numDataPoints = Ybuffer.size();
	g.numModelPoints = Xbuffer.size();
}
inline void cleanupBuffers() { step_globals().reg.reset(); }
}  // namespace PointCloud

namespace ICP {
inline void require_buffers()
{
	if (!step_globals().reg) throw std::runtime_error("ICP step: PointCloud::initBuffers was not called");
}
// one ICP iteration on the device-resident clouds (exact NN through the engine's own tree in both forms)
inline void naiveGPUStep()
{
	require_buffers();
	check(goicp_icp_step(step_globals().reg->handle()));
}
// kdTreeGPUStep(KDTree&, PointCloudAdaptor&, FlattenedKDTree*): the reference's host / flattened trees are not needed
template <class... TreeArgs>
inline void kdTreeGPUStep(TreeArgs&&...) { naiveGPUStep(); }
// CPUStep(dataBuffer, modelBuffer): one iteration, then the caller's data vector is moved as the reference does in place
template <class Point3>
inline void CPUStep(std::vector<Point3>& dataBuffer, std::vector<Point3>& modelBuffer)
{
	StepGlobals& g = step_globals();
	if (!g.reg) PointCloud::initBuffers(dataBuffer, modelBuffer);
	if (dataBuffer.size() != g.numDataPoints) throw std::invalid_argument("ICP::CPUStep: data buffer size changed");
	naiveGPUStep();
	goicp_result r;
	check(goicp_poll(g.reg->handle(), &r));
	static_assert(sizeof(Point3) == 3 * sizeof(float), "Point3 must be three packed floats");
	check(goicp_transform_source(g.reg->handle(), r.curR, r.curT, reinterpret_cast<float*>(dataBuffer.data())));
}
// accumulated pose of the step API and the source cloud under it (what the viewer draws)
inline void step_pose(Mat3& R, Vec3& t)
{
	require_buffers();
	goicp_result r;
	check(goicp_poll(step_globals().reg->handle(), &r));
	R = from_rows(r.curR); t = from_xyz(r.curT);
}
template <class Point3>
inline void step_positions(std::vector<Point3>& out)
{
	require_buffers();
	StepGlobals& g = step_globals();
	goicp_result r;
	check(goicp_poll(g.reg->handle(), &r));
	out.resize(g.numDataPoints);
	check(goicp_transform_source(g.reg->handle(), r.curR, r.curT, reinterpret_cast<float*>(out.data())));
}
// goicpGPUStep(fgoicp, prev_optR, prev_optT, mtx) (src/goicp_kernel.cu:152-206): the viewer's poll.  Returns whether the
// optimum changed (the reference redraws in that case); sets the global goicp_finished exactly as the reference does.
inline bool goicpGPUStep(const icp::FastGoICP* fgoicp, Mat3& prev_optR, Vec3& prev_optT, std::mutex& mtx)
{
	StepGlobals& g = step_globals();
	bool updated;
	float currentError;
	{
		std::lock_guard<std::mutex> lock(mtx);
		g.goicp_finished = fgoicp->finished;
		updated = (prev_optR != fgoicp->optR || prev_optT != fgoicp->optT);
		currentError = fgoicp->get_best_error();
		prev_optR = fgoicp->optR;
		prev_optT = fgoicp->optT;
	}
	float thr = g.sse_threshold;
	if (thr <= 0.f) goicp_thresholds(fgoicp->registration.handle(), &thr, nullptr);
	if (currentError <= thr) g.goicp_finished = true;
	return updated;
}
}  // namespace ICP

}  // namespace goicp_mi355
