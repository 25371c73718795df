// C ABI of libgoicp_mi355.so (declared in include/goicp_mi355.h): exception -> status translation
// around goicp::Engine and the config / cloud IO helpers.
#include "../../include/goicp_mi355.h"

#include <climits>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "comm.hpp"
#include "config_io.hpp"
#include "engine.hpp"

struct goicp_engine {
	goicp::Engine* e;
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
	g_err = msg;
	return code;
}

template <class F> int guarded(F&& f)
{
	try {
		f();
		return GOICP_OK;
	} catch (const goicp::StatusError& e) { return fail(e.rc, e.what());
	} catch (const goicp::ConfigError& e) { return fail(GOICP_ERR_CONFIG, e.what());
	} catch (const goicp::IoError& e) { return fail(GOICP_ERR_IO, e.what());
	} catch (const std::invalid_argument& e) { return fail(GOICP_ERR_INVALID, e.what());
	} catch (const std::bad_alloc&) { return fail(GOICP_ERR_INTERNAL, "out of host memory");
	} catch (const std::runtime_error& e) {
		std::string m = e.what();
		return fail(m.find("no HIP device") != std::string::npos ? GOICP_ERR_NO_DEVICE : GOICP_ERR_DEVICE, m);
	} catch (const std::exception& e) { return fail(GOICP_ERR_INTERNAL, e.what());
	} catch (...) { return fail(GOICP_ERR_INTERNAL, "unknown error"); }
}

#define REQUIRE(c) do { if (!(c)) return fail(GOICP_ERR_INVALID, std::string(__func__) + ": invalid argument (" #c ")"); } while (0)

void fill_counters(goicp_counters* o, const goicp::Counters& c)
{
	o->rot_pops = c.rot_pops; o->trans_pops = c.trans_pops; o->cubes = c.cubes; o->inner_calls = c.inner_calls;
	o->icp_runs = c.icp_runs; o->icp_iters = c.icp_iters; o->bounds_launches = c.bounds_launches; o->queue_fallbacks = c.queue_fallbacks;
	o->tile_expansions = c.tile_expansions; o->lane_batches = c.lane_batches;
}

void fill_result(goicp_result* out, const goicp::Result& r)
{
	std::memcpy(out->optR, r.optR, sizeof(r.optR)); std::memcpy(out->optT, r.optT, sizeof(r.optT));
	std::memcpy(out->curR, r.curR, sizeof(r.curR)); std::memcpy(out->curT, r.curT, sizeof(r.curT));
	out->best_sse = r.best_sse; out->finished = r.finished;
	fill_counters(&out->counters, r.counters);
	out->dt_build_ms = r.dt_build_ms; out->register_ms = r.register_ms;
}

}  // namespace

extern "C" {

const char* goicp_last_error(void) { return g_err.c_str(); }
int goicp_abi_version(void) { return GOICP_ABI_VERSION; }
#ifndef GOICP_KERNEL_HASH
#define GOICP_KERNEL_HASH "unknown"
#endif
const char* goicp_kernel_source_hash(void) { return GOICP_KERNEL_HASH; }

int goicp_config_load(const char* toml_path, goicp_config* out)
{
	REQUIRE(toml_path && out);
	return guarded([&] { goicp::load_config(toml_path, out); });
}

int goicp_cloud_load(const char* path, float subsample, float resize, uint64_t seed, float** xyz, size_t* n)
{
	REQUIRE(path && xyz && n);
	*xyz = nullptr; *n = 0;
	return guarded([&] {
		std::vector<float> v;
		goicp::load_cloud(path, subsample, resize, seed, v);
		float* p = new float[v.size() ? v.size() : 1];
		std::memcpy(p, v.data(), v.size() * sizeof(float));
		*xyz = p; *n = v.size() / 3;
	});
}

void goicp_cloud_free(float* xyz) { delete[] xyz; }

void goicp_params_default(goicp_params* p)
{
	if (!p) return;
	goicp::Params d;
	p->dt_size = d.dt_size; p->dt_expand = d.dt_expand; p->mse_threshold = d.mse_threshold; p->dt_layout = d.dt_layout;
	p->device = d.device; p->trans_batch = d.trans_batch; p->wide_children = d.wide_children;
	p->icp_max_iter = d.icp_max_iter; p->verbose = d.verbose; p->morton_sort = d.morton_sort; p->rot_batch = d.rot_batch; p->trim_fraction = d.trim_fraction; p->kd_gpu_build = d.kd_gpu_build;
	p->use_rot_range = d.use_rot_range; p->use_trans_range = d.use_trans_range;
	for (int k = 0; k < 3; k++) {
		p->rot_min[k] = d.rot_min[k]; p->rot_max[k] = d.rot_max[k];
		p->trans_min[k] = d.trans_min[k]; p->trans_max[k] = d.trans_max[k];
	}
	p->rot_search_depth = d.rot_search_depth; p->trans_search_depth = d.trans_search_depth;
	p->icp_fused = d.icp_fused; p->bounds_fp16 = d.bounds_fp16; p->icp_nn_cache = d.icp_nn_cache; p->flow = d.flow; p->adaptive_k = d.adaptive_k; p->queue_cap = d.queue_cap; p->device_queues = d.device_queues;
	p->lds_tiles = d.lds_tiles; p->tile_spread_vox = d.tile_spread_vox; p->tile_min = d.tile_min; p->stale_widen = d.stale_widen; p->ub_tiebreak = d.ub_tiebreak; p->icp_point_seed = d.icp_point_seed; p->ub_share = d.ub_share; p->twin_fusion = d.twin_fusion; p->sort_items = d.sort_items; p->stale_compact = d.stale_compact; p->stream_priority = d.stream_priority; p->lanes = d.lanes; p->lane_min_searches = d.lane_min_searches;
	p->bounds_order = d.bounds_order; p->bounds_order_min_groups = d.bounds_order_min_groups; p->bounds_order_max_runs = d.bounds_order_max_runs; p->bounds_order_cell = d.bounds_order_cell; p->bounds_order_reprobe = d.bounds_order_reprobe;
	p->bounds_balance = d.bounds_balance; p->bounds_balance_a = d.bounds_balance_a; p->bounds_dedup = d.bounds_dedup;
}

void goicp_params_from_config(const goicp_config* c, goicp_params* p)
{
	if (!p) return;
	goicp_params_default(p);
	if (!c) return;
	p->mse_threshold = c->mse_threshold;
	if (c->has_rotation_range) {
		p->use_rot_range = 1;
		for (int k = 0; k < 3; k++) { p->rot_min[k] = c->rot_min[k]; p->rot_max[k] = c->rot_max[k]; }
		p->rot_search_depth = c->rot_search_depth;
	}
	if (c->has_translation_range) {
		p->use_trans_range = 1;
		for (int k = 0; k < 3; k++) { p->trans_min[k] = c->trans_min[k]; p->trans_max[k] = c->trans_max[k]; }
		p->trans_search_depth = c->trans_search_depth;
	}
}

int goicp_create(const goicp_params* params, const float* target_xyz, size_t n_target, const float* source_xyz,
                 size_t n_source, goicp_handle* out)
{
	REQUIRE(out);
	*out = nullptr;
	REQUIRE(target_xyz && source_xyz && n_target > 0 && n_source > 0);
	return guarded([&] {
		goicp::Params p;
		if (params) {
			p.dt_size = params->dt_size; p.dt_expand = params->dt_expand; p.mse_threshold = params->mse_threshold;
			p.dt_layout = params->dt_layout; p.device = params->device; p.trans_batch = params->trans_batch;
			p.wide_children = params->wide_children; p.icp_max_iter = params->icp_max_iter; p.verbose = params->verbose;
			p.morton_sort = params->morton_sort;
			if (params->rot_batch > 0) p.rot_batch = params->rot_batch;
			p.trim_fraction = params->trim_fraction;
			p.kd_gpu_build = params->kd_gpu_build;
			p.use_rot_range = params->use_rot_range; p.use_trans_range = params->use_trans_range;
			for (int k = 0; k < 3; k++) {
				p.rot_min[k] = params->rot_min[k]; p.rot_max[k] = params->rot_max[k];
				p.trans_min[k] = params->trans_min[k]; p.trans_max[k] = params->trans_max[k];
			}
			p.rot_search_depth = params->rot_search_depth; p.trans_search_depth = params->trans_search_depth;
			p.icp_fused = params->icp_fused; p.bounds_fp16 = params->bounds_fp16; p.icp_nn_cache = params->icp_nn_cache; p.flow = params->flow; p.adaptive_k = params->adaptive_k; p.queue_cap = params->queue_cap; p.device_queues = params->device_queues;
			p.lds_tiles = params->lds_tiles; p.stale_widen = params->stale_widen; p.ub_tiebreak = params->ub_tiebreak; p.icp_point_seed = params->icp_point_seed; p.ub_share = params->ub_share; p.twin_fusion = params->twin_fusion; p.sort_items = params->sort_items; p.stale_compact = params->stale_compact; p.stream_priority = params->stream_priority; p.lanes = params->lanes; p.lane_min_searches = params->lane_min_searches;
			p.bounds_order = params->bounds_order; p.bounds_order_min_groups = params->bounds_order_min_groups; p.bounds_order_max_runs = params->bounds_order_max_runs; p.bounds_order_reprobe = params->bounds_order_reprobe;
			p.bounds_balance = params->bounds_balance; p.bounds_balance_a = params->bounds_balance_a; p.bounds_dedup = params->bounds_dedup;
			if (params->bounds_order_cell > 0.f) p.bounds_order_cell = params->bounds_order_cell;
			if (params->tile_spread_vox > 0.f) p.tile_spread_vox = params->tile_spread_vox;
			if (params->tile_min > 0) p.tile_min = params->tile_min;
		}
		goicp_engine* h = new goicp_engine{nullptr};
		try { h->e = new goicp::Engine(p, target_xyz, n_target, source_xyz, n_source); }
		catch (...) { delete h; throw; }
		*out = h;
	});
}

int goicp_destroy(goicp_handle h)
{
	if (!h) return GOICP_OK;
	return guarded([&] { delete h->e; delete h; });
}

int goicp_set_source(goicp_handle h, const float* source_xyz, size_t n_source)
{
	REQUIRE(h && source_xyz && n_source > 0);
	return guarded([&] { h->e->set_source(source_xyz, n_source); });
}

int goicp_source_order_host(const float* xyz, size_t n, int32_t mode, int32_t* perm)
{
	REQUIRE(xyz && perm && n > 0 && mode >= 0 && mode <= 2);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::source_order_host(xyz, n, mode, perm); });
}

int goicp_debug_source_order(goicp_handle h, const float* xyz, size_t n, int32_t mode, int32_t* perm)
{
	REQUIRE(h && xyz && perm && n > 0);
	return guarded([&] { h->e->debug_source_order(xyz, n, mode, perm); });
}

int goicp_voxel_downsample_host(const float* xyz, size_t n, float voxel, float* out_xyz, int32_t* out_count, size_t* m)
{
	REQUIRE(xyz && out_xyz && m && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::voxel_downsample_host(xyz, n, voxel, out_xyz, out_count, m); });
}

int goicp_voxel_downsample(goicp_handle h, const float* xyz, size_t n, float voxel, float* out_xyz, int32_t* out_count, size_t* m)
{
	REQUIRE(h && xyz && out_xyz && m && n > 0);
	return guarded([&] { h->e->voxel_downsample(xyz, n, voxel, out_xyz, out_count, m); });
}

int goicp_set_source_voxel(goicp_handle h, const float* xyz, size_t n, float voxel, size_t* n_kept)
{
	REQUIRE(h && xyz && n > 0 && voxel != 0.f);          // this entry point has no "no stage": a voxel of 0 is as bad as a negative one
	goicp::Engine::SourceStages st;
	st.voxel = voxel;
	return guarded([&] { h->e->set_source_staged("goicp_set_source_voxel", xyz, n, st, n_kept); });
}

int goicp_radius_outlier_removal_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, float* out_xyz, int32_t* out_index,
                                      int32_t* out_count, size_t* m)
{
	REQUIRE(xyz && out_xyz && m && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::radius_outlier_removal_host(xyz, n, radius, min_neighbors, out_xyz, out_index, out_count, m); });
}

int goicp_radius_outlier_removal(goicp_handle h, const float* xyz, size_t n, float radius, int32_t min_neighbors, float* out_xyz, int32_t* out_index,
                                 int32_t* out_count, size_t* m)
{
	REQUIRE(h && xyz && out_xyz && m && n > 0);
	return guarded([&] { h->e->radius_outlier_removal(xyz, n, radius, min_neighbors, out_xyz, out_index, out_count, m); });
}

void goicp_source_filter_default(goicp_source_filter* out)
{
	if (!out) return;
	out->voxel = 0.f;
	out->radius = 0.f;
	out->min_neighbors = 0;
}

int goicp_set_source_filtered(goicp_handle h, const float* xyz, size_t n, const goicp_source_filter* f, size_t* n_kept)
{
	REQUIRE(h && xyz && f && n > 0);
	goicp::Engine::SourceStages st;
	st.voxel = f->voxel;
	st.radius = f->radius;
	st.min_neighbors = f->min_neighbors;
	return guarded([&] { h->e->set_source_staged("goicp_set_source_filtered", xyz, n, st, n_kept); });
}

int goicp_statistical_outlier_removal_host(const float* xyz, size_t n, int32_t neighbors, float std_ratio, float* out_xyz, int32_t* out_index,
                                           float* out_mean_dist, double* threshold, size_t* m)
{
	REQUIRE(xyz && out_xyz && m && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::statistical_outlier_removal_host(xyz, n, neighbors, std_ratio, out_xyz, out_index, out_mean_dist, threshold, m); });
}

int goicp_statistical_outlier_removal(goicp_handle h, const float* xyz, size_t n, int32_t neighbors, float std_ratio, float* out_xyz, int32_t* out_index,
                                      float* out_mean_dist, double* threshold, size_t* m)
{
	REQUIRE(h && xyz && out_xyz && m && n > 0);
	return guarded([&] { h->e->statistical_outlier_removal(xyz, n, neighbors, std_ratio, out_xyz, out_index, out_mean_dist, threshold, m); });
}

void goicp_source_pipeline_default(goicp_source_pipeline* out)
{
	if (!out) return;
	out->voxel = 0.f;
	out->stat_neighbors = 0;
	out->stat_std_ratio = 0.f;
	out->radius = 0.f;
	out->min_neighbors = 0;
}

// the first three stages of the chain, as the C struct names them
static goicp::Engine::SourceStages stages_of(const goicp_source_pipeline& p)
{
	goicp::Engine::SourceStages st;
	st.voxel = p.voxel;
	st.stat_neighbors = p.stat_neighbors;
	st.stat_std_ratio = p.stat_std_ratio;
	st.radius = p.radius;
	st.min_neighbors = p.min_neighbors;
	return st;
}

int goicp_set_source_pipeline(goicp_handle h, const float* xyz, size_t n, const goicp_source_pipeline* p, size_t* n_kept)
{
	REQUIRE(h && xyz && p && n > 0);
	return guarded([&] { h->e->set_source_staged("goicp_set_source_pipeline", xyz, n, stages_of(*p), n_kept); });
}

int goicp_cluster_host(const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t* out_label, int32_t* out_sizes, size_t* n_clusters)
{
	REQUIRE(xyz && out_label && n_clusters && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::cluster_host(xyz, n, radius, min_neighbors, out_label, out_sizes, n_clusters); });
}

int goicp_cluster(goicp_handle h, const float* xyz, size_t n, float radius, int32_t min_neighbors, int32_t* out_label, int32_t* out_sizes, size_t* n_clusters)
{
	REQUIRE(h && xyz && out_label && n_clusters && n > 0);
	return guarded([&] { h->e->cluster(xyz, n, radius, min_neighbors, out_label, out_sizes, n_clusters); });
}

void goicp_cluster_select_default(goicp_cluster_select* out)
{
	if (!out) return;
	out->radius = 0.f;
	out->min_neighbors = 0;
	out->min_size = 0;
	out->max_clusters = 0;
}

int goicp_cluster_filter_host(const float* xyz, size_t n, const goicp_cluster_select* s, float* out_xyz, int32_t* out_index, int32_t* out_label, size_t* m)
{
	REQUIRE(xyz && s && out_xyz && m && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::cluster_filter_host(xyz, n, s->radius, s->min_neighbors, s->min_size, s->max_clusters, out_xyz, out_index, out_label, m); });
}

int goicp_cluster_filter(goicp_handle h, const float* xyz, size_t n, const goicp_cluster_select* s, float* out_xyz, int32_t* out_index, int32_t* out_label,
                         size_t* m)
{
	REQUIRE(h && xyz && s && out_xyz && m && n > 0);
	return guarded([&] { h->e->cluster_filter(xyz, n, s->radius, s->min_neighbors, s->min_size, s->max_clusters, out_xyz, out_index, out_label, m); });
}

int goicp_set_source_clustered(goicp_handle h, const float* xyz, size_t n, const goicp_source_pipeline* p, const goicp_cluster_select* s, size_t* n_kept)
{
	REQUIRE(h && xyz && s && n > 0);
	goicp::Engine::SourceStages st;
	if (p) st = stages_of(*p);
	st.cluster_radius = s->radius;
	st.cluster_min_neighbors = s->min_neighbors;
	st.cluster_min_size = s->min_size;
	st.cluster_max_clusters = s->max_clusters;
	return guarded([&] { h->e->set_source_staged("goicp_set_source_clustered", xyz, n, st, n_kept); });
}

void goicp_plane_select_default(goicp_plane_select* out)
{
	if (!out) return;
	out->distance = 0.f;
	out->iterations = 0;
	out->refine = 0;
	out->max_planes = 0;
	out->min_inliers = 0;
	out->seed = 0;
}

static_assert(sizeof(goicp_plane) == sizeof(goicp::PlaneRecord) && sizeof(goicp_plane) == 40, "goicp_plane is PlaneRecord, field for field");
static goicp::PlaneRecord* records(goicp_plane* p) { return reinterpret_cast<goicp::PlaneRecord*>(p); }
static goicp::PlaneSelect checked(const goicp_plane_select& s)
{
	return goicp::plane_check_select(s.distance, s.iterations, s.refine, s.max_planes, s.min_inliers, s.seed);
}

int goicp_segment_plane_host(const float* xyz, size_t n, const goicp_plane_select* sel, int32_t* out_label, goicp_plane* out_planes, size_t* n_planes)
{
	REQUIRE(xyz && sel && out_label && out_planes && n_planes && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] {
		const goicp::PlaneSelect s = checked(*sel);
		goicp::plane_check_cloud(xyz, n);
		goicp::segment_plane_host(xyz, n, s, out_label, nullptr, nullptr, records(out_planes), n_planes, nullptr);
	});
}

int goicp_segment_plane(goicp_handle h, const float* xyz, size_t n, const goicp_plane_select* sel, int32_t* out_label, goicp_plane* out_planes, size_t* n_planes)
{
	REQUIRE(h && xyz && sel && out_label && out_planes && n_planes && n > 0);
	return guarded([&] { h->e->segment_plane(xyz, n, checked(*sel), out_label, records(out_planes), n_planes); });
}

int goicp_plane_filter_host(const float* xyz, size_t n, const goicp_plane_select* sel, float* out_xyz, int32_t* out_index, goicp_plane* out_planes,
                            size_t* n_planes, size_t* m)
{
	REQUIRE(xyz && sel && out_xyz && m && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] {
		const goicp::PlaneSelect s = checked(*sel);
		goicp::plane_check_cloud(xyz, n);
		goicp::segment_plane_host(xyz, n, s, nullptr, out_xyz, out_index, records(out_planes), n_planes, m);
	});
}

int goicp_plane_filter(goicp_handle h, const float* xyz, size_t n, const goicp_plane_select* sel, float* out_xyz, int32_t* out_index, goicp_plane* out_planes,
                       size_t* n_planes, size_t* m)
{
	REQUIRE(h && xyz && sel && out_xyz && m && n > 0);
	return guarded([&] { h->e->plane_filter(xyz, n, checked(*sel), out_xyz, out_index, records(out_planes), n_planes, m); });
}

int goicp_set_source_segmented(goicp_handle h, const float* xyz, size_t n, const goicp_source_pipeline* p, const goicp_plane_select* pl,
                               const goicp_cluster_select* s, size_t* n_kept)
{
	REQUIRE(h && xyz && n > 0);
	goicp::Engine::SourceStages st;
	if (p) st = stages_of(*p);
	if (pl) {
		st.plane_distance = pl->distance;
		st.plane_iterations = pl->iterations;
		st.plane_refine = pl->refine;
		st.plane_max = pl->max_planes;
		st.plane_min_inliers = pl->min_inliers;
		st.plane_seed = pl->seed;
	}
	if (s) {
		st.cluster_radius = s->radius;
		st.cluster_min_neighbors = s->min_neighbors;
		st.cluster_min_size = s->min_size;
		st.cluster_max_clusters = s->max_clusters;
	}
	return guarded([&] { h->e->set_source_staged("goicp_set_source_segmented", xyz, n, st, n_kept); });
}

int goicp_knn_self_host(const float* xyz, size_t n, int32_t k, int32_t* out_index, float* out_dist_sq)
{
	REQUIRE(xyz && out_index && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::knn_self_host(xyz, n, k, out_index, out_dist_sq); });
}

int goicp_knn_self(goicp_handle h, const float* xyz, size_t n, int32_t k, int32_t* out_index, float* out_dist_sq)
{
	REQUIRE(h && xyz && out_index && n > 0);
	return guarded([&] { h->e->knn_self(xyz, n, k, out_index, out_dist_sq); });
}

int goicp_estimate_normals_host(const float* xyz, size_t n, int32_t k, const float vp[3], float* out_normals, float* out_variation, int32_t* out_index)
{
	REQUIRE(xyz && out_normals && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::estimate_normals_host(xyz, n, k, vp, out_normals, out_variation, out_index); });
}

int goicp_estimate_normals(goicp_handle h, const float* xyz, size_t n, int32_t k, const float vp[3], float* out_normals, float* out_variation,
                           int32_t* out_index)
{
	REQUIRE(h && xyz && out_normals && n > 0);
	return guarded([&] { h->e->estimate_normals(xyz, n, k, vp, out_normals, out_variation, out_index); });
}

int goicp_fpfh_host(const float* xyz, const float* normals, size_t n, int32_t k, float* out_fpfh, uint8_t* out_spfh_counts)
{
	REQUIRE(xyz && normals && out_fpfh && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::fpfh_host(xyz, normals, n, k, out_fpfh, out_spfh_counts); });
}

int goicp_fpfh(goicp_handle h, const float* xyz, const float* normals, size_t n, int32_t k, float* out_fpfh, uint8_t* out_spfh_counts)
{
	REQUIRE(h && xyz && normals && out_fpfh && n > 0);
	REQUIRE(n <= (size_t)INT32_MAX / 8);
	return guarded([&] { h->e->fpfh(xyz, normals, n, k, out_fpfh, out_spfh_counts); });
}

int goicp_match_features_host(const float* query, size_t n_q, const float* target, size_t n_t, int32_t* out_index, float* out_d2, float* out_d2_second,
                              uint8_t* out_mutual)
{
	REQUIRE(query && target && out_index && out_d2 && out_d2_second && n_q > 0 && n_t > 0);
	REQUIRE(n_q <= (size_t)INT32_MAX / 8 && n_t <= (size_t)INT32_MAX / 8);
	return guarded([&] { goicp::match_features_host(query, n_q, target, n_t, out_index, out_d2, out_d2_second, out_mutual); });
}

int goicp_match_features(goicp_handle h, const float* query, size_t n_q, const float* target, size_t n_t, int32_t* out_index, float* out_d2,
                         float* out_d2_second, uint8_t* out_mutual)
{
	REQUIRE(h && query && target && out_index && out_d2 && out_d2_second && n_q > 0 && n_t > 0);
	REQUIRE(n_q <= (size_t)INT32_MAX / 8 && n_t <= (size_t)INT32_MAX / 8);
	return guarded([&] { h->e->match_features(query, n_q, target, n_t, out_index, out_d2, out_d2_second, out_mutual); });
}

int goicp_match_features_tile(void) { return goicp::kMatchTile; }

void goicp_ransac_pose_select_default(goicp_ransac_pose_select* out)
{
	if (!out) return;
	out->distance = 0.f;
	out->iterations = 0;
	out->refine = 1;
	out->max_poses = 0;
	out->min_inliers = 0;
	out->edge_similarity = 0.9f;
	out->seed = 0;
}

static_assert(sizeof(goicp_ransac_pose_result) == sizeof(goicp::RansacPoseRecord) && sizeof(goicp_ransac_pose_result) == 60, "goicp_ransac_pose_result is RansacPoseRecord, field for field");
static goicp::RansacPoseRecord* records(goicp_ransac_pose_result* p) { return reinterpret_cast<goicp::RansacPoseRecord*>(p); }
static goicp::RansacPoseSelect checked(const goicp_ransac_pose_select& s)
{
	return goicp::ransac_pose_check_select(s.distance, s.iterations, s.refine, s.max_poses, s.min_inliers, s.edge_similarity, s.seed);
}

int goicp_ransac_pose_host(const float* src, size_t n_s, const float* tgt, size_t n_t, const int32_t* corr, size_t M, const goicp_ransac_pose_select* sel,
                           goicp_ransac_pose_result* out_poses, size_t* n_poses, uint8_t* out_inlier)
{
	REQUIRE(src && tgt && corr && sel && out_poses && n_poses);
	return guarded([&] {
		const goicp::RansacPoseSelect s = checked(*sel);
		goicp::ransac_pose_check_input(src, n_s, tgt, n_t, corr, M);
		goicp::ransac_pose_host(src, tgt, corr, M, s, records(out_poses), n_poses, out_inlier);
	});
}

int goicp_ransac_pose(goicp_handle h, const float* src, size_t n_s, const float* tgt, size_t n_t, const int32_t* corr, size_t M,
                      const goicp_ransac_pose_select* sel, goicp_ransac_pose_result* out_poses, size_t* n_poses, uint8_t* out_inlier)
{
	REQUIRE(h && src && tgt && corr && sel && out_poses && n_poses);
	return guarded([&] { h->e->ransac_pose(src, n_s, tgt, n_t, corr, M, checked(*sel), records(out_poses), n_poses, out_inlier); });
}

int goicp_select_matches(const int32_t* index, const float* d2, const float* d2_second, const uint8_t* mutual, size_t n_q, float ratio, int32_t require_mutual,
                         int32_t* out_corr, size_t* M)
{
	REQUIRE(index && d2 && d2_second && out_corr && M);
	return guarded([&] { goicp::select_matches_host(index, d2, d2_second, mutual, n_q, ratio, require_mutual, out_corr, M); });
}

int goicp_ransac_pose_tile(void) { return goicp::kRpTile; }
int goicp_ransac_pose_block(void) { return goicp::kRpBlock * goicp::kRpPts; }

int goicp_thresholds(goicp_handle h, float* sse_threshold, int32_t* inliers)
{
	REQUIRE(h);
	if (sse_threshold) *sse_threshold = h->e->sse_threshold();
	if (inliers) *inliers = h->e->inliers();
	return GOICP_OK;
}

int goicp_device(goicp_handle h, int32_t* ordinal)
{
	REQUIRE(h && ordinal);
	*ordinal = h->e->device();
	return GOICP_OK;
}

int goicp_set_progress_callback(goicp_handle h, goicp_progress_fn cb, void* user)
{
	REQUIRE(h);
	if (!cb) { h->e->set_progress_callback(nullptr); return GOICP_OK; }
	h->e->set_progress_callback([cb, user](const goicp::Result& r) {
		goicp_result out;
		fill_result(&out, r);
		cb(&out, user);
	});
	return GOICP_OK;
}

int goicp_probe_gather(goicp_handle h, int32_t mode, size_t window_bytes, double* lookups_per_s)
{
	REQUIRE(h && lookups_per_s && (mode == 0 || mode == 1 || mode == 2 || mode == 4 || mode == 8 || mode == 16 || mode == 32));
	return guarded([&] { *lookups_per_s = h->e->probe_gather(mode, window_bytes); });
}

int goicp_debug_cache_hits(goicp_handle h, const float R[9], const float t[3], int64_t* hits)
{
	REQUIRE(h && R && t && hits);
	return guarded([&] { *hits = h->e->debug_cache_hits(R, t); });
}

int goicp_debug_bounds_tile(goicp_handle h, const float* rots9, const float* parents4, int32_t nseg, int32_t n, int32_t level, int32_t chunks,
                            float* ub_tile, float* lb_tile, float* ub_direct, float* lb_direct, float ms[2], uint32_t stats[2])
{
	REQUIRE(h && rots9 && parents4 && ub_tile && lb_tile && ub_direct && lb_direct && ms && stats);
	return guarded([&] { h->e->debug_bounds_tile(rots9, parents4, nseg, n, level, chunks, ub_tile, lb_tile, ub_direct, lb_direct, ms, stats); });
}

int goicp_debug_queue_expand(goicp_handle h, const float R[9], int32_t level, const float* parents4, int32_t n, float* ub_ubpass, float* lb_ubpass,
                             float* ub_lbpass, float* lb_lbpass, int32_t info[2])
{
	REQUIRE(h && R && parents4 && ub_ubpass && lb_ubpass && ub_lbpass && lb_lbpass && info && n >= 1);
	return guarded([&] {
		int inf[2] = {0, 0};
		h->e->debug_queue_expand(R, level, parents4, n, ub_ubpass, lb_ubpass, ub_lbpass, lb_lbpass, inf);
		info[0] = inf[0]; info[1] = inf[1];
	});
}

int goicp_debug_queue_expand_tiles(goicp_handle h, const float R[9], int32_t level, const float* parents4, int32_t n, int32_t n_ub, float* ub_ubpass,
                                   float* lb_ubpass, float* ub_lbpass, float* lb_lbpass, int32_t info[4], int32_t digest, float* queue_nodes,
                                   int32_t* queue_counts, float* listed4, float* search8)
{
	REQUIRE(h && R && parents4 && ub_ubpass && lb_ubpass && ub_lbpass && lb_lbpass && info && n >= 1 && n_ub >= 1 && n_ub <= n);
	REQUIRE(!digest || (queue_nodes && queue_counts && listed4 && search8));
	return guarded([&] {
		int inf[4] = {0, 0, 0, 0}, counts[4] = {0, 0, 0, 0};
		const goicp::Engine::QueueDigest dg{queue_nodes, counts, listed4, search8};
		h->e->debug_queue_expand_tiles(R, level, parents4, n, n_ub, ub_ubpass, lb_ubpass, ub_lbpass, lb_lbpass, inf, digest ? &dg : nullptr);
		for (int k = 0; k < 4; k++) info[k] = inf[k];
		if (digest) for (int k = 0; k < 4; k++) queue_counts[k] = counts[k];
	});
}

int goicp_debug_queue_round(goicp_handle h, const goicp_queue_round* round, goicp_queue_search* searches, float* nodes, const void* prev_parents,
                            const float* prev_ub, const float* prev_lb, const float* prev_scratch, int32_t ctl[6], void* listed,
                            int32_t* parent_search)
{
	REQUIRE(h && round && searches && nodes && ctl && listed);
	return guarded([&] { h->e->debug_queue_round(*round, searches, nodes, prev_parents, prev_ub, prev_lb, prev_scratch, ctl, listed, parent_search); });
}

int goicp_debug_bounds_order(goicp_handle h, int32_t info[3])
{
	REQUIRE(h && info);
	return guarded([&] {
		int inf[3] = {0, 0, 0};
		h->e->debug_bounds_order(inf);
		info[0] = inf[0]; info[1] = inf[1]; info[2] = inf[2];
	});
}

int goicp_debug_bounds_twins(goicp_handle h, int32_t info[2])
{
	REQUIRE(h && info);
	return guarded([&] {
		int inf[2] = {0, 0};
		h->e->debug_bounds_twins(inf);
		info[0] = inf[0]; info[1] = inf[1];
	});
}

int goicp_debug_bounds_copies(goicp_handle h, int32_t info[1])
{
	REQUIRE(h && info);
	return guarded([&] {
		int inf[1] = {0};
		h->e->debug_bounds_copies(inf);
		info[0] = inf[0];
	});
}

int goicp_debug_bounds_balance(goicp_handle h, int32_t info[26])
{
	REQUIRE(h && info);
	return guarded([&] {
		int inf[26];
		h->e->debug_bounds_balance(inf);
		for (int k = 0; k < 26; k++) info[k] = inf[k];
	});
}

int goicp_debug_bounds_xcd_spans(goicp_handle h, uint64_t out[96])
{
	REQUIRE(h && out);
	static_assert(goicp::kXcdStampRows * goicp::kXcdStampCols == 96, "goicp_debug_bounds_xcd_spans: 96 words");
	return guarded([&] {
		unsigned long long w[96];
		if (!h->e->debug_bounds_xcd_spans(w)) throw std::invalid_argument("goicp_debug_bounds_xcd_spans: not a diagnostic build (GOICP_BOUNDS_XCD_STAMPS)");
		for (int k = 0; k < 96; k++) out[k] = w[k];
	});
}

int goicp_debug_select(goicp_handle h, const float* d2, size_t n, int32_t num, int32_t kernel, uint8_t* include)
{
	REQUIRE(h && d2 && include && n >= 1 && n <= 0x7fffffffu && num >= 1 && (size_t)num <= n && kernel >= 0 && kernel <= 2 && !(kernel == 1 && n > 32768));
	return guarded([&] { h->e->debug_select(d2, n, num, kernel, include); });
}

int goicp_debug_kabsch(const float H[9], float R[9])
{
	REQUIRE(H && R);
	return guarded([&] { goicp::debug_kabsch(H, R); });
}

int goicp_dt_info(goicp_handle h, int32_t* V, double* scale, double origin[3])
{
	REQUIRE(h);
	const goicp::DtDesc& d = h->e->dt();
	if (V) *V = d.V;
	if (scale) *scale = d.scale;
	if (origin) { origin[0] = d.xmin; origin[1] = d.ymin; origin[2] = d.zmin; }
	return GOICP_OK;
}

int goicp_dt_download(goicp_handle h, float* grid)
{
	REQUIRE(h && grid);
	return guarded([&] { h->e->dt_download(grid); });
}

int goicp_eval_bounds(goicp_handle h, const float R[9], const float* cubes, size_t B, int32_t level, float* ub, float* lb)
{
	REQUIRE(h && R && (B == 0 || (cubes && ub && lb)));
	return guarded([&] { h->e->eval_bounds(R, cubes, B, level, ub, lb); });
}

int goicp_eval_bounds_batch(goicp_handle h, const float* rots, size_t K, const goicp_cube* cubes, size_t B, float* ub, float* lb)
{
	REQUIRE(h && (B == 0 || (rots && K > 0 && cubes && ub && lb)));
	static_assert(sizeof(goicp_cube) == sizeof(goicp::CubeRec), "goicp_cube layout");
	return guarded([&] { h->e->eval_bounds_batch(rots, K, reinterpret_cast<const goicp::CubeRec*>(cubes), B, ub, lb); });
}

int goicp_eval_bounds_device(goicp_handle h, const void* d_rots, const void* d_cubes, size_t B, void* d_ub, void* d_lb, void* stream)
{
	REQUIRE(h && d_rots && d_cubes && d_ub && d_lb && B > 0);
	return guarded([&] {
		h->e->eval_bounds_dev(static_cast<const goicp::Rot9*>(d_rots), static_cast<const goicp::CubeRec*>(d_cubes), (int)B,
		                      static_cast<float*>(d_ub), static_cast<float*>(d_lb), static_cast<hipStream_t>(stream));
	});
}

int goicp_eval_bounds_device_grouped(goicp_handle h, const void* d_rots, size_t n_rots, const void* d_cubes, size_t B, void* d_ub, void* d_lb, void* stream)
{
	REQUIRE(h && d_rots && d_cubes && d_ub && d_lb && B > 0 && n_rots >= 1 && n_rots <= 16);
	return guarded([&] {
		h->e->eval_bounds_dev_grouped(static_cast<const goicp::Rot9*>(d_rots), (int)n_rots, static_cast<const goicp::CubeRec*>(d_cubes), (int)B,
		                              static_cast<float*>(d_ub), static_cast<float*>(d_lb), static_cast<hipStream_t>(stream));
	});
}

int goicp_time_bounds_device_grouped(goicp_handle h, const void* d_rots, size_t n_rots, const void* d_cubes, size_t B, void* d_ub, void* d_lb, int32_t iters, float* ms)
{
	REQUIRE(h && d_rots && d_cubes && d_ub && d_lb && B > 0 && iters > 0 && ms && n_rots >= 1 && n_rots <= 16);
	return guarded([&] {
		*ms = h->e->time_bounds_dev(static_cast<const goicp::Rot9*>(d_rots), static_cast<const goicp::CubeRec*>(d_cubes), (int)B, static_cast<float*>(d_ub),
		                            static_cast<float*>(d_lb), iters, (int)n_rots);
	});
}

int goicp_reduce_min_device(goicp_handle h, const void* d_values, size_t n, void* d_min, void* d_argmin, void* stream)
{
	REQUIRE(h && d_values && d_min && n > 0 && n <= 0x7fffffffu && ((uintptr_t)d_values & 15) == 0);
	return guarded([&] {
		h->e->reduce_min_dev(static_cast<const float*>(d_values), (int)n, static_cast<float*>(d_min), static_cast<int*>(d_argmin), static_cast<hipStream_t>(stream));
	});
}

int goicp_time_bounds_device(goicp_handle h, const void* d_rots, const void* d_cubes, size_t B, void* d_ub, void* d_lb,
                             int32_t iters, float* ms)
{
	REQUIRE(h && d_rots && d_cubes && d_ub && d_lb && B > 0 && iters > 0 && ms);
	return guarded([&] {
		*ms = h->e->time_bounds_dev(static_cast<const goicp::Rot9*>(d_rots), static_cast<const goicp::CubeRec*>(d_cubes),
		                            (int)B, static_cast<float*>(d_ub), static_cast<float*>(d_lb), iters);
	});
}

float goicp_rot_coeff(goicp_handle h, int32_t level) { return h ? h->e->rot_coeff(level) : 0.f; }
float goicp_trans_delta(float w) { return (float)(1.732050808 / 2.0 * (double)w); }
void goicp_rodrigues(const float v[3], float R[9]) { if (v && R) goicp::rodrigues(v[0], v[1], v[2], R); }

int goicp_eval_sse(goicp_handle h, const float R[9], const float t[3], float* sse)
{
	REQUIRE(h && R && t && sse);
	return guarded([&] { *sse = h->e->eval_sse(R, t); });
}

int goicp_inner_bnb(goicp_handle h, const float R[9], int32_t level, float incumbent, float* value, float best_node[4],
                    goicp_counters* counters)
{
	REQUIRE(h && R && value);
	return guarded([&] {
		goicp::Counters c;
		*value = h->e->inner_bnb(R, level, incumbent, best_node, &c);
		if (counters) fill_counters(counters, c);
	});
}

int goicp_icp_run(goicp_handle h, float R[9], float t[3], int32_t max_iter, float err_diff, float* err, int32_t* iters)
{
	REQUIRE(h && R && t && max_iter >= 0);
	return guarded([&] {
		int it = 0;
		float e = h->e->icp_run(R, t, max_iter, err_diff, &it);
		if (err) *err = e;
		if (iters) *iters = it;
	});
}

int goicp_icp_run_batch(goicp_handle h, size_t K, float* R, float* t, int32_t max_iter, float err_diff, float* err, int32_t* iters)
{
	REQUIRE(h && R && t && max_iter >= 0 && K >= 1 && K <= (size_t)goicp::kIcpBatchMax);
	return guarded([&] { h->e->icp_run_batch(K, R, t, max_iter, err_diff, err, iters); });
}

int goicp_icp_run_collective(goicp_handle h, const goicp_comm_ops* comm, float R[9], float t[3], int32_t max_iter, float err_diff, float* err,
                             int32_t* iters)
{
	REQUIRE(h && comm && comm->allreduce_min_u64 && comm->bcast && R && t && max_iter >= 0);
	g_err.clear();
	int rc = GOICP_ERR_INTERNAL;
	const int g = guarded([&] {
		int it = 0;
		float e = 0.f;
		rc = h->e->icp_run_collective(comm, R, t, max_iter, err_diff, &e, &it);
		if (rc == GOICP_OK) {
			if (err) *err = e;
			if (iters) *iters = it;
		}
	});
	if (g != GOICP_OK) return g;
	if (rc == GOICP_ERR_TIMEOUT) g_err = "collective ICP: a collective missed the communicator's deadline (a rank is lost); exit non-zero";
	else if (rc == GOICP_ERR_PEER) g_err = "collective ICP: another rank reported a failure";
	else if (rc != GOICP_OK && g_err.empty()) g_err = "collective ICP failed";
	return rc;
}

int goicp_icp_shard_stats_get(goicp_handle h, goicp_icp_shard_stats* out)
{
	REQUIRE(h && out);
	const goicp::IcpShardStats& s = h->e->icp_shard_stats();
	out->rank = s.rank; out->world = s.world;
	out->block_begin = s.block_begin; out->block_end = s.block_end; out->blocks = s.blocks; out->sliced = s.sliced;
	out->queries = s.queries; out->runs = s.runs; out->passes = s.passes; out->collectives = s.collectives;
	out->sum_wait_ms = s.sum_wait_ms; out->round_trip_ms = s.round_trip_ms;
	return GOICP_OK;
}

int goicp_time_icp_pass(goicp_handle h, const float R[9], const float t[3], int32_t iters, float* ms)
{
	REQUIRE(h && R && t && iters > 0 && ms);
	return guarded([&] { *ms = h->e->time_icp_pass(R, t, iters); });
}

int goicp_time_icp_pass_cached(goicp_handle h, const float R[9], const float t[3], int32_t iters, float* ms)
{
	REQUIRE(h && R && t && iters > 0 && ms);
	return guarded([&] { *ms = h->e->time_icp_pass(R, t, iters, true); });
}

int goicp_nn_query(goicp_handle h, const float* q, size_t n, int32_t* index, float* dist_sq)
{
	REQUIRE(h && (n == 0 || (q && index && dist_sq)));
	return guarded([&] { h->e->nn_query(q, n, index, dist_sq); });
}

void goicp_icp_options_default(goicp_icp_options* out)
{
	if (!out) return;
	out->metric = 0;
	out->normal_k = 16;
}

int goicp_set_icp_options(goicp_handle h, const goicp_icp_options* opt)
{
	REQUIRE(h && opt);
	return guarded([&] { h->e->set_icp_options(opt->metric, opt->normal_k); });
}

void goicp_icp_gate_default(goicp_icp_gate* out)
{
	if (!out) return;
	out->max_corr_dist = 0.f;
	out->min_inliers = 0;
	out->capped_walk = 1;
}

int goicp_set_icp_gate(goicp_handle h, const goicp_icp_gate* gate)
{
	REQUIRE(gate);
	// what the struct alone decides is refused before the handle is looked at
	REQUIRE(gate->max_corr_dist >= 0.f && gate->max_corr_dist <= 3.402823466e+38f);
	REQUIRE(gate->min_inliers == 0 || gate->min_inliers >= 3);
	REQUIRE(gate->capped_walk == 0 || gate->capped_walk == 1);
	REQUIRE(h);
	return guarded([&] { h->e->set_icp_gate(gate->max_corr_dist, gate->min_inliers, gate->capped_walk); });
}

void goicp_icp_robust_default(goicp_icp_robust* out)
{
	if (!out) return;
	out->kernel = 0;
	out->scale = 0.f;
}

int goicp_set_icp_robust(goicp_handle h, const goicp_icp_robust* r)
{
	REQUIRE(r && h);
	return guarded([&] { h->e->set_icp_robust(r->kernel, r->scale); });
}

int goicp_set_search_truncation(goicp_handle h, float max_dist)
{
	// what the distance alone decides is refused before the handle is looked at
	REQUIRE(max_dist >= 0.f && max_dist <= 3.402823466e+38f);
	REQUIRE(h);
	return guarded([&] { h->e->set_search_truncation(max_dist); });
}

int goicp_search_truncation(goicp_handle h, float* max_dist)
{
	REQUIRE(h && max_dist);
	return guarded([&] { *max_dist = h->e->search_truncation(); });
}

int goicp_icp_robust_stats(goicp_handle h, size_t K, float* cost, float* weight_sum)
{
	REQUIRE(h && K >= 1);
	return guarded([&] { h->e->icp_robust_stats(K, cost, weight_sum); });
}

int goicp_icp_inliers(goicp_handle h, size_t K, int32_t* inliers)
{
	REQUIRE(h && inliers && K >= 1);
	return guarded([&] { h->e->icp_inliers(K, inliers); });
}

int goicp_eval_correspondences(goicp_handle h, const float R[9], const float t[3], float max_corr_dist, int32_t* index, float* dist_sq, int32_t* inliers,
                               float* sse_inliers)
{
	REQUIRE(max_corr_dist >= 0.f && max_corr_dist <= 3.402823466e+38f);
	REQUIRE(h && R && t);
	return guarded([&] { h->e->eval_correspondences(R, t, max_corr_dist, index, dist_sq, inliers, sse_inliers); });
}

int goicp_knn_query(goicp_handle h, const float* q, size_t n, int32_t k, int32_t* index, float* dist_sq)
{
	REQUIRE(h && (n == 0 || (q && index && dist_sq)));
	return guarded([&] { h->e->knn_query(q, n, k, index, dist_sq); });
}

int goicp_target_normals(goicp_handle h, float* normals_xyz)
{
	REQUIRE(h && normals_xyz);
	return guarded([&] { h->e->target_normals(normals_xyz); });
}

int goicp_set_icp_symmetric(goicp_handle h, int32_t enabled, int32_t source_normal_k)
{
	REQUIRE(h);
	return guarded([&] { h->e->set_icp_symmetric(enabled, source_normal_k); });
}

int goicp_get_icp_symmetric(goicp_handle h, int32_t* enabled, int32_t* source_normal_k, int32_t* user_normals)
{
	REQUIRE(h && enabled && source_normal_k && user_normals);
	return guarded([&] {
		h->e->check_symmetric_query("goicp_get_icp_symmetric");
		*enabled = h->e->icp_symmetric() ? 1 : 0;
		*source_normal_k = h->e->source_normal_k();
		*user_normals = h->e->user_source_normals() ? 1 : 0;
	});
}

int goicp_set_icp_generalized(goicp_handle h, int32_t enabled, float epsilon, int32_t source_normal_k)
{
	REQUIRE(h);
	return guarded([&] { h->e->set_icp_generalized(enabled, epsilon, source_normal_k); });
}

int goicp_get_icp_generalized(goicp_handle h, int32_t* enabled, float* epsilon, int32_t* source_normal_k, int32_t* user_normals)
{
	REQUIRE(h && enabled && epsilon && source_normal_k && user_normals);
	return guarded([&] {
		h->e->check_symmetric_query("goicp_get_icp_generalized");
		*enabled = h->e->icp_generalized() ? 1 : 0;
		*epsilon = h->e->gicp_epsilon();
		*source_normal_k = h->e->source_normal_k();
		*user_normals = h->e->user_source_normals() ? 1 : 0;
	});
}

int goicp_source_normals(goicp_handle h, float* normals_xyz)
{
	REQUIRE(h && normals_xyz);
	return guarded([&] { h->e->source_normals(normals_xyz); });
}

int goicp_set_source_normals(goicp_handle h, const float* normals_xyz, size_t n)
{
	REQUIRE(h && normals_xyz);
	return guarded([&] { h->e->set_source_normals(normals_xyz, n); });
}

void goicp_pose_info_options_default(goicp_pose_info_options* out)
{
	if (!out) return;
	out->metric = -1;
	out->use_pivot = 0;
	out->pivot[0] = out->pivot[1] = out->pivot[2] = 0.0;
	out->rank_tol = goicp::Engine::kPoseInfoRankTol;
}

int goicp_pose_information(goicp_handle h, const float R[9], const float t[3], const goicp_pose_info_options* opt, goicp_pose_info* out)
{
	REQUIRE(h && R && t && out);
	return guarded([&] { h->e->pose_information(1, R, t, opt, out, false); });
}

int goicp_pose_information_batch(goicp_handle h, size_t K, const float* R, const float* t, const goicp_pose_info_options* opt, goicp_pose_info* out)
{
	REQUIRE(h);                 // K and the pointers are refused by name below
	return guarded([&] { h->e->pose_information(K, R, t, opt, out, true); });
}

int goicp_result_information(goicp_handle h, const goicp_pose_info_options* opt, goicp_pose_info* out)
{
	REQUIRE(h && out);
	return guarded([&] { h->e->result_information(opt, out); });
}

int goicp_information_decompose(const double info[36], double rank_tol, double eig[6], double vec[36], double pinv[36], int32_t* rank)
{
	REQUIRE(info);
	return guarded([&] { goicp::information_decompose(info, rank_tol, eig, vec, pinv, rank); });
}

int goicp_icp_step(goicp_handle h)
{
	REQUIRE(h);
	return guarded([&] { h->e->icp_step(); });
}

int goicp_register(goicp_handle h)
{
	REQUIRE(h);
	return guarded([&] { h->e->run(); });
}

int goicp_cancel(goicp_handle h)
{
	REQUIRE(h);
	h->e->cancel();
	return GOICP_OK;
}

int goicp_poll(goicp_handle h, goicp_result* out)
{
	REQUIRE(h && out);
	return guarded([&] {
		fill_result(out, h->e->poll());
	});
}

int goicp_result_write_toml(goicp_handle h, const char* path)
{
	REQUIRE(h && path);
	return guarded([&] { goicp::write_result_toml(path, h->e->poll(), h->e->n_source(), h->e->n_target(), h->e->sse_threshold(), h->e->inliers()); });
}

int goicp_result_write_ply(goicp_handle h, const char* path)
{
	REQUIRE(h && path);
	return guarded([&] {
		goicp::Result r = h->e->poll();
		std::vector<float> moved(3 * h->e->n_source());
		h->e->source_transformed(r.optR, r.optT, moved.data());
		goicp::write_viz_ply(path, h->e->target_xyz(), h->e->n_target(), moved.data(), h->e->n_source());
	});
}

int goicp_transform_source(goicp_handle h, const float R[9], const float t[3], float* out_xyz)
{
	REQUIRE(h && R && t && out_xyz);
	return guarded([&] { h->e->source_transformed(R, t, out_xyz); });
}

int goicp_set_shard(goicp_handle h, int32_t rank, int32_t world)
{
	REQUIRE(h && world >= 1 && rank >= 0 && rank < world);
	h->e->set_shard(rank, world);
	return GOICP_OK;
}

int goicp_register_begin(goicp_handle h)
{
	REQUIRE(h);
	return guarded([&] { h->e->register_begin(); });
}

int goicp_register_step(goicp_handle h, int32_t max_rot_pops, goicp_step_status* out)
{
	REQUIRE(h && out && max_rot_pops > 0);
	return guarded([&] {
		goicp::StepStatus s = h->e->register_step(max_rot_pops);
		out->finished = s.finished; out->early_exit = s.early_exit; out->best_sse = s.best_sse;
		out->frontier_lb = s.frontier_lb; out->rot_pops = s.rot_pops;
	});
}

int goicp_offer_best(goicp_handle h, float sse, const float R[9], const float t[3])
{
	REQUIRE(h && R && t);
	return guarded([&] { h->e->offer_global_best(sse, R, t); });
}

int goicp_register_end(goicp_handle h)
{
	REQUIRE(h);
	return guarded([&] { h->e->register_end(); });
}

// ---- sharded registration: the engine as the protocol's callback table ---------------------------------------------
namespace {
goicp::Engine* E(void* ctx) { return static_cast<goicp_engine*>(ctx)->e; }
int eo_begin(void* c, int32_t rank, int32_t world) { return guarded([&] { E(c)->set_shard(rank, world); E(c)->register_begin(); }); }
int eo_step(void* c, int32_t max_pops, goicp_step_status* out) { return goicp_register_step(static_cast<goicp_engine*>(c), max_pops, out); }
int eo_pose(void* c, float* sse, float R[9], float t[3])
{
	return guarded([&] {
		const goicp::Result r = E(c)->poll();
		*sse = r.best_sse;
		std::memcpy(R, r.optR, sizeof(r.optR));
		std::memcpy(t, r.optT, sizeof(r.optT));
	});
}
int eo_offer(void* c, float sse, const float R[9], const float t[3]) { return guarded([&] { E(c)->offer_global_best(sse, R, t); }); }
int eo_qsize(void* c, int32_t* n) { return guarded([&] { *n = E(c)->queue_size(); }); }
int eo_donate(void* c, int32_t max_nodes, float* nodes7, int32_t* n) { return guarded([&] { *n = E(c)->donate(max_nodes, nodes7); }); }
int eo_receive(void* c, const float* nodes7, int32_t n) { return guarded([&] { E(c)->receive(nodes7, n); }); }
int eo_end(void* c) { return guarded([&] { E(c)->register_end(); }); }
int eo_unrefined(void* c, int32_t* flag) { return guarded([&] { *flag = E(c)->pose_unrefined() ? 1 : 0; }); }
int eo_refine(void* c, const float pose[12], float* sse, float R[9], float t[3])
{
	return guarded([&] {
		std::memcpy(R, pose, sizeof(float) * 9);
		std::memcpy(t, pose + 9, sizeof(float) * 3);
		*sse = E(c)->refine_collective(R, t);
	});
}
}  // namespace

void goicp_shard_options_default(goicp_shard_options* out)
{
	if (!out) return;
	// the step follows the single-GPU driver's ramp up to 32 parents per batch: measured on 1/2/4/8 ranks (tools/shard_inflation.py) the
	// prove-the-optimum run inflates by 1.02 (4 ranks) / 1.10 (8) with it, in a quarter of the exchanges of a fixed 8
	out->rot_pops_per_step = 8; out->rebalance = 1; out->stale_exchange = 0; out->ramp_to = 32;
}

int goicp_run_sharded_opt(const goicp_shard_engine_ops* engine, const goicp_comm_ops* comm, const goicp_shard_options* opt, goicp_shard_stats* stats)
{
	REQUIRE(engine && comm && opt && engine->begin && engine->step && engine->pose && engine->offer && engine->queue_size && engine->donate &&
	        engine->receive && engine->end && comm->allreduce_min_u64 && comm->bcast && opt->rot_pops_per_step >= 1);
	g_err.clear();                  // a message left by an earlier, unrelated failure on this thread must not be reported for this run
	int rc = GOICP_ERR_INTERNAL;
	const int g = guarded([&] { rc = goicp::run_sharded(engine, comm, opt, stats); });
	if (g != GOICP_OK) return g;
	if (rc == GOICP_ERR_TIMEOUT) g_err = "sharded registration: a collective missed the communicator's deadline (a rank is lost); exit non-zero";
	else if (rc == GOICP_ERR_PEER) g_err = "sharded registration: rank " + std::to_string(stats ? stats->failed_rank : -1) + " reported a failure";
	else if (rc != GOICP_OK && g_err.empty()) g_err = "sharded registration: a callback failed";
	return rc;
}

int goicp_run_sharded(const goicp_shard_engine_ops* engine, const goicp_comm_ops* comm, int32_t rot_pops_per_step, int32_t rebalance,
                      goicp_shard_stats* stats)
{
	goicp_shard_options o;
	goicp_shard_options_default(&o);
	o.rot_pops_per_step = rot_pops_per_step; o.rebalance = rebalance;
	return goicp_run_sharded_opt(engine, comm, &o, stats);
}

int goicp_register_sharded_opt(goicp_handle h, const goicp_comm_ops* comm, const goicp_shard_options* opt, goicp_shard_stats* stats)
{
	REQUIRE(h && comm && opt);
	goicp_shard_engine_ops eo{};
	eo.ctx = h; eo.sse_threshold = h->e->sse_threshold();
	eo.begin = eo_begin; eo.step = eo_step; eo.pose = eo_pose; eo.offer = eo_offer; eo.queue_size = eo_qsize;
	eo.donate = eo_donate; eo.receive = eo_receive; eo.end = eo_end;
	return goicp_run_sharded_opt(&eo, comm, opt, stats);
}

int goicp_register_sharded_collective_icp(goicp_handle h, const goicp_comm_ops* comm, const goicp_shard_options* opt, goicp_shard_stats* stats)
{
	REQUIRE(h && comm && opt && comm->allreduce_min_u64 && comm->bcast && opt->rot_pops_per_step >= 1);
	if (opt->stale_exchange) return fail(GOICP_ERR_INVALID, "goicp_register_sharded_collective_icp: stale_exchange would interleave the refinements' collectives with the exchange");
	goicp_shard_engine_ops eo{};
	eo.ctx = h; eo.sse_threshold = h->e->sse_threshold();
	eo.begin = eo_begin; eo.step = eo_step; eo.pose = eo_pose; eo.offer = eo_offer; eo.queue_size = eo_qsize;
	eo.donate = eo_donate; eo.receive = eo_receive; eo.end = eo_end;
	const goicp::ShardIcpHooks hooks{eo_unrefined, eo_refine};
	struct Scope {
		goicp::Engine* e;
		~Scope() { e->set_collective_icp(nullptr); }
	} scope{h->e};
	h->e->set_collective_icp(comm);
	g_err.clear();
	int rc = GOICP_ERR_INTERNAL;
	const int g = guarded([&] { rc = goicp::run_sharded(&eo, comm, opt, stats, &hooks); });
	if (g != GOICP_OK) return g;
	if (rc == GOICP_ERR_TIMEOUT) g_err = "sharded registration: a collective missed the communicator's deadline (a rank is lost); exit non-zero";
	else if (rc == GOICP_ERR_PEER) g_err = "sharded registration: rank " + std::to_string(stats ? stats->failed_rank : -1) + " reported a failure";
	else if (rc != GOICP_OK && g_err.empty()) g_err = "sharded registration: a callback failed";
	return rc;
}

int goicp_register_sharded(goicp_handle h, const goicp_comm_ops* comm, int32_t rot_pops_per_step, int32_t rebalance, goicp_shard_stats* stats)
{
	goicp_shard_options o;
	goicp_shard_options_default(&o);
	o.rot_pops_per_step = rot_pops_per_step; o.rebalance = rebalance;
	return goicp_register_sharded_opt(h, comm, &o, stats);
}

int goicp_comm_set_timeout_ms(goicp_comm_ops* comm, int32_t timeout_ms)
{
	REQUIRE(comm && comm->ctx && timeout_ms >= 1);
	const int rc = goicp::comm_set_timeout_ms(comm, timeout_ms);
	return rc == GOICP_OK ? rc : fail(rc, "goicp_comm_set_timeout_ms: not a communicator made by this library");
}

int goicp_comm_allreduce_sum_i64(const goicp_comm_ops* comm, int64_t* words, size_t n)
{
	REQUIRE(comm && comm->allreduce_min_u64 && comm->bcast && (words || n == 0));
	const int rc = goicp::comm_allreduce_sum_i64(comm, words, n);
	if (rc == GOICP_ERR_TIMEOUT) return fail(rc, "goicp_comm_allreduce_sum_i64: the communicator's deadline passed");
	return rc == GOICP_OK ? rc : fail(rc, "goicp_comm_allreduce_sum_i64 failed");
}

int goicp_thread_comm_create(int32_t world, goicp_comm_ops* out)
{
	REQUIRE(out && world >= 1 && world <= 1024);
	return guarded([&] { if (goicp::thread_comm_create(world, out) != GOICP_OK) throw std::bad_alloc(); });
}
int goicp_thread_comm_destroy(goicp_comm_ops* comm) { goicp::thread_comm_destroy(comm); return GOICP_OK; }

int goicp_rccl_unique_id(char id128[GOICP_RCCL_ID_BYTES])
{
	REQUIRE(id128);
	const int rc = goicp::rccl_unique_id(id128);
	return rc == GOICP_OK ? rc : fail(rc, "ncclGetUniqueId failed");
}

int goicp_rccl_comm_create(const char id128[GOICP_RCCL_ID_BYTES], int32_t rank, int32_t world, int32_t device, goicp_comm_ops* out)
{
	REQUIRE(id128 && out && world >= 1 && rank >= 0 && rank < world && device >= 0);
	const int rc = goicp::rccl_comm_create(id128, rank, world, device, out);
	return rc == GOICP_OK ? rc : fail(rc, "RCCL communicator creation failed (ncclCommInitRank / staging buffers)");
}

int goicp_rccl_comm_wrap(void* nccl_comm, int32_t rank, int32_t world, int32_t device, goicp_comm_ops* out)
{
	REQUIRE(nccl_comm && out && world >= 1 && rank >= 0 && rank < world && device >= 0);
	const int rc = goicp::rccl_comm_wrap(nccl_comm, rank, world, device, out);
	return rc == GOICP_OK ? rc : fail(rc, "RCCL communicator staging buffers could not be created");
}

int goicp_rccl_comm_destroy(goicp_comm_ops* comm) { return goicp::rccl_comm_destroy(comm); }

int goicp_register_multi_gpu(const goicp_params* params, const float* target_xyz, size_t n_target, const float* source_xyz, size_t n_source,
                             int32_t world, int32_t rot_pops_per_step, goicp_handle* out, goicp_shard_stats* stats)
{
	REQUIRE(out && target_xyz && source_xyz && n_target > 0 && n_source > 0 && world >= 1 && world <= 64 && rot_pops_per_step >= 1);
	*out = nullptr;
	goicp_params base;
	if (params) base = *params; else goicp_params_default(&base);
	std::vector<goicp_handle> hs((size_t)world, nullptr);
	std::vector<void*> raw((size_t)world, nullptr);
	std::vector<goicp_comm_ops> comms((size_t)world);
	std::vector<int> rcs((size_t)world, GOICP_OK);
	std::vector<std::string> errs((size_t)world);
	int rc = GOICP_OK;
	auto cleanup = [&](bool keep0) {
		for (int r = 0; r < world; r++) {
			goicp_rccl_comm_destroy(&comms[(size_t)r]);
			goicp::rccl_comm_destroy_raw(raw[(size_t)r]);
			if (!(keep0 && r == 0)) goicp_destroy(hs[(size_t)r]);
		}
	};
	for (int r = 0; r < world; r++) std::memset(&comms[(size_t)r], 0, sizeof(goicp_comm_ops));
	// one engine per GPU, created side by side (DT + k-d builds overlap)
	{
		std::vector<std::thread> th;
		for (int r = 0; r < world; r++)
			th.emplace_back([&, r] {
				goicp_params p = base;
				p.device = r;
				rcs[(size_t)r] = goicp_create(&p, target_xyz, n_target, source_xyz, n_source, &hs[(size_t)r]);
				if (rcs[(size_t)r] != GOICP_OK) errs[(size_t)r] = goicp_last_error();
			});
		for (auto& t : th) t.join();
	}
	for (int r = 0; r < world; r++) if (rcs[(size_t)r] != GOICP_OK) { rc = rcs[(size_t)r]; g_err = errs[(size_t)r]; }
	if (rc == GOICP_OK && goicp::rccl_comm_init_all(world, raw.data()) != GOICP_OK) rc = fail(GOICP_ERR_DEVICE, "ncclCommInitAll failed");
	for (int r = 0; rc == GOICP_OK && r < world; r++) rc = goicp_rccl_comm_wrap(raw[(size_t)r], r, world, r, &comms[(size_t)r]);
	if (rc != GOICP_OK) { cleanup(false); return rc; }
	{
		std::vector<std::thread> th;
		for (int r = 0; r < world; r++)
			th.emplace_back([&, r] {
				rcs[(size_t)r] = goicp_register_sharded(hs[(size_t)r], &comms[(size_t)r], rot_pops_per_step, 1, stats ? &stats[r] : nullptr);
				if (rcs[(size_t)r] != GOICP_OK) errs[(size_t)r] = goicp_last_error();
			});
		for (auto& t : th) t.join();
	}
	for (int r = 0; r < world; r++) if (rcs[(size_t)r] != GOICP_OK) { rc = rcs[(size_t)r]; g_err = errs[(size_t)r]; }
	cleanup(rc == GOICP_OK);
	if (rc == GOICP_OK) *out = hs[0];
	return rc;
}

}  // extern "C"
