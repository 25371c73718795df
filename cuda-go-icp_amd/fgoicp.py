"""Python mirrors of the reference's operator interface for this path, over the C ABI.

Reference classes mirrored (names, argument meaning, error behaviour):
  Config                      src/common.h:133-180, src/common.cpp:12-77
  load_cloud                  src/common.cpp:205-228
  icp::RotNode / TransNode    src/fgoicp/fgoicp_common.hpp:64-129 (here with the CPU path's
                              corner+width parametrisation, src/goicp/jly_goicp.h:44-72)
  icp::Registration           src/fgoicp/registration.hpp:44-98
  icp::IterativeClosestPoint3D  src/fgoicp/icp3d.hpp:9-41
  icp::FastGoICP              src/fgoicp/fgoicp.hpp:11-69
All compute happens in libgoicp_mi355.so on the GPU; these classes only marshal arguments.
"""
import ctypes as C
import threading

import numpy as np

from . import binding as B


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _pose_info_options(metric=None, pivot=None, rank_tol=None):
    o = B.CPoseInfoOptions()
    B.load_library().goicp_pose_info_options_default(C.byref(o))
    if metric is not None:
        o.metric = int(metric)
    if pivot is not None:
        pv = np.asarray(pivot, np.float64).reshape(3)
        o.use_pivot = 1
        o.pivot[:] = [float(x) for x in pv]
    if rank_tol is not None:
        o.rank_tol = float(rank_tol)
    return o


def _pose_info_dict(i):
    """goicp_pose_info -> dict of numpy arrays and scalars (the struct's field names)"""
    return {"information": np.array(i.information, np.float64).reshape(6, 6), "gradient": np.array(i.gradient, np.float64),
            "covariance": np.array(i.covariance, np.float64).reshape(6, 6), "eigenvalues": np.array(i.eigenvalues, np.float64),
            "eigenvectors": np.array(i.eigenvectors, np.float64).reshape(6, 6), "pivot": np.array(i.pivot, np.float64),
            "weight_sum": float(i.weight_sum), "cost": float(i.cost), "sse": float(i.sse), "sigma2": float(i.sigma2),
            "inliers": int(i.inliers), "rank": int(i.rank), "metric": int(i.metric), "dof_nonpositive": int(i.dof_nonpositive)}


def information_decompose(A, rank_tol=1e-6):
    """goicp_information_decompose (host only): symmetric 6x6 -> (eigenvalues ascending (6,), eigenvectors as rows (6, 6), pinv (6, 6), rank)"""
    A = np.ascontiguousarray(A, np.float64).reshape(36)
    eig, vec, pinv, rank = np.empty(6), np.empty(36), np.empty(36), C.c_int32()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    B.check(B.load_library().goicp_information_decompose(dp(A), float(rank_tol), dp(eig), dp(vec), dp(pinv), C.byref(rank)))
    return eig, vec.reshape(6, 6), pinv.reshape(6, 6), rank.value


def source_order(xyz, mode=2):
    """goicp_source_order_host (host only): the permutation the engine orders a source cloud by (goicp_params.morton_sort = mode: 0 input
    order, 1 Morton curve, 2 k-d order); perm[sorted position] = original index.  The device ordering of goicp_set_source equals it."""
    xyz = _f32(xyz, (-1, 3))
    perm = np.empty(len(xyz), np.int32)
    B.check(B.load_library().goicp_source_order_host(_fptr(xyz), len(xyz), int(mode), perm.ctypes.data_as(C.POINTER(C.c_int32))))
    return perm


def _voxel_call(fn, xyz, voxel):
    xyz = _f32(xyz, (-1, 3))
    out, cnt, m = np.empty((len(xyz), 3), np.float32), np.empty(len(xyz), np.int32), C.c_size_t(0)
    B.check(fn(_fptr(xyz), len(xyz), float(voxel), _fptr(out), cnt.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m)))
    return out[:m.value].copy(), cnt[:m.value].copy()


def voxel_downsample(xyz, voxel):
    """goicp_voxel_downsample_host (host only): one centroid per occupied cell of a grid of pitch `voxel`, cells in ascending key order ->
    (cloud (m, 3) float32, counts (m,) int32).  Registration.voxel_downsample and set_source(voxel=) give the same bits on the device."""
    return _voxel_call(B.load_library().goicp_voxel_downsample_host, xyz, voxel)


def _outlier_call(fn, xyz, radius, min_neighbors):
    xyz = _f32(xyz, (-1, 3))
    n, ip = len(xyz), C.POINTER(C.c_int32)
    out, idx, cnt, m = np.empty((n, 3), np.float32), np.empty(n, np.int32), np.empty(n, np.int32), C.c_size_t(0)
    B.check(fn(_fptr(xyz), n, float(radius), int(min_neighbors), _fptr(out), idx.ctypes.data_as(ip), cnt.ctypes.data_as(ip), C.byref(m)))
    return out[:m.value].copy(), idx[:m.value].copy(), cnt


def radius_outlier_removal(xyz, radius, min_neighbors):
    """goicp_radius_outlier_removal_host (host only): the points with at least `min_neighbors` other points within `radius`, in input order
    -> (cloud (m, 3) float32, their indices (m,) int32, min(neighbours, min_neighbors) of every input point (n,) int32).
    Registration.radius_outlier_removal and set_source(radius=, min_neighbors=) give the same bits on the device."""
    return _outlier_call(B.load_library().goicp_radius_outlier_removal_host, xyz, radius, min_neighbors)


def _stat_call(fn, xyz, neighbors, std_ratio):
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    out, idx, mean, thr, m = np.empty((n, 3), np.float32), np.empty(n, np.int32), np.empty(n, np.float32), C.c_double(0.0), C.c_size_t(0)
    B.check(fn(_fptr(xyz), n, int(neighbors), float(std_ratio), _fptr(out), idx.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(mean), C.byref(thr), C.byref(m)))
    return out[:m.value].copy(), idx[:m.value].copy(), mean, thr.value


def statistical_outlier_removal(xyz, neighbors, std_ratio):
    """goicp_statistical_outlier_removal_host (host only): the points whose mean distance to their `neighbors` nearest neighbours is at most
    the cloud's mean of it plus `std_ratio` sample deviations, in input order -> (cloud (m, 3) float32, their indices (m,) int32, the mean
    distance of every input point (n,) float32, the threshold as a float).  Registration.statistical_outlier_removal and
    set_source(stat_neighbors=, std_ratio=) give the same bits on the device."""
    return _stat_call(B.load_library().goicp_statistical_outlier_removal_host, xyz, neighbors, std_ratio)


def _knn_self_call(fn, xyz, k):
    xyz = _f32(xyz, (-1, 3))
    n, k = len(xyz), int(k)
    idx, d2 = np.empty((n, max(k, 0)), np.int32), np.empty((n, max(k, 0)), np.float32)
    B.check(fn(_fptr(xyz), n, k, idx.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(d2)))
    return idx, d2


def knn_self(xyz, k):
    """goicp_knn_self_host (host only): the k nearest OTHER points of every point of the cloud, exact, ascending by (d2, index) ->
    (indices (n, k) int32, squared distances (n, k) float32).  Registration.knn_self gives the same bits on the device."""
    return _knn_self_call(B.load_library().goicp_knn_self_host, xyz, k)


def _normals_call(fn, xyz, k, viewpoint):
    xyz = _f32(xyz, (-1, 3))
    n, k = len(xyz), int(k)
    vp = None if viewpoint is None else _f32(viewpoint, (3,))
    nrm, var, idx = np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty((n, max(k - 1, 0)), np.int32)
    B.check(fn(_fptr(xyz), n, k, None if vp is None else _fptr(vp), _fptr(nrm), _fptr(var), idx.ctypes.data_as(C.POINTER(C.c_int32))))
    return nrm, var, idx


def estimate_normals(xyz, k, viewpoint=None):
    """goicp_estimate_normals_host (host only): per-point normals and surface variation from the k-point neighbourhood (the point itself and
    its k - 1 nearest others), flipped towards `viewpoint` when one is given -> (normals (n, 3) float32, variation (n,) float32, the
    neighbours used (n, k - 1) int32).  Registration.estimate_normals gives the same bits on the device."""
    return _normals_call(B.load_library().goicp_estimate_normals_host, xyz, k, viewpoint)


FPFH_DIM = 33


def _fpfh_call(fn, xyz, normals, k):
    xyz, normals = _f32(xyz, (-1, 3)), _f32(normals, (-1, 3))
    if len(normals) != len(xyz):
        raise ValueError("fpfh: one normal per point")
    n = len(xyz)
    out, cnt = np.empty((n, FPFH_DIM), np.float32), np.empty((n, FPFH_DIM), np.uint8)
    B.check(fn(_fptr(xyz), _fptr(normals), n, int(k), _fptr(out), cnt.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out, cnt


def fpfh(xyz, k, normals=None, normal_k=16, viewpoint=None):
    """goicp_fpfh_host (host only): the 33-bin FPFH descriptor of every point from its k nearest other points and the normals (the
    caller's, or estimate_normals(xyz, normal_k, viewpoint) when none are given) -> (descriptors (n, 33) float32, SPFH counts (n, 33)
    uint8).  Registration.fpfh gives the same bits on the device."""
    if normals is None:
        normals = estimate_normals(xyz, normal_k, viewpoint)[0]
    return _fpfh_call(B.load_library().goicp_fpfh_host, xyz, normals, k)


def _match_call(fn, fq, ft, mutual):
    fq, ft = _f32(fq, (-1, FPFH_DIM)), _f32(ft, (-1, FPFH_DIM))
    nq = len(fq)
    idx, d2, second = np.empty(nq, np.int32), np.empty(nq, np.float32), np.empty(nq, np.float32)
    mut = np.empty(nq, np.uint8) if mutual else None
    B.check(fn(_fptr(fq), nq, _fptr(ft), len(ft), idx.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(d2), _fptr(second),
               mut.ctypes.data_as(C.POINTER(C.c_uint8)) if mutual else None))
    return idx, d2, second, mut


def match_features(fq, ft, mutual=True):
    """goicp_match_features_host (host only): for every query descriptor the nearest target descriptor in the 33-dimensional space, ties
    to the smaller index -> (indices (n_q,) int32, squared distances (n_q,) float32, the second-nearest squared distances (n_q,) float32,
    mutual flags (n_q,) uint8 or None).  The cost is n_q * n_t: meant for downsampled clouds.  Registration.match_features gives the same
    bits on the device."""
    return _match_call(B.load_library().goicp_match_features_host, fq, ft, mutual)


def _cluster_call(fn, xyz, radius, min_neighbors):
    xyz = _f32(xyz, (-1, 3))
    n, ip = len(xyz), C.POINTER(C.c_int32)
    label, sizes, c = np.empty(n, np.int32), np.empty(n, np.int32), C.c_size_t(0)
    B.check(fn(_fptr(xyz), n, float(radius), int(min_neighbors), label.ctypes.data_as(ip), sizes.ctypes.data_as(ip), C.byref(c)))
    return label, sizes[:c.value].copy()


def cluster(xyz, radius, min_neighbors=0):
    """goicp_cluster_host (host only): connected components of the core points under `radius` (min_neighbors = 0: every point is core,
    Euclidean clustering; >= 1: DBSCAN with min_points = min_neighbors + 1), border points joined to their nearest core neighbour ->
    (labels (n,) int32, -1 = noise, sizes (c,) int32).  Registration.cluster gives the same bits on the device."""
    return _cluster_call(B.load_library().goicp_cluster_host, xyz, radius, min_neighbors)


def _cluster_filter_call(fn, xyz, radius, min_neighbors, min_size, keep):
    xyz = _f32(xyz, (-1, 3))
    n, ip = len(xyz), C.POINTER(C.c_int32)
    out, idx, lab, m = np.empty((n, 3), np.float32), np.empty(n, np.int32), np.empty(n, np.int32), C.c_size_t(0)
    s = B.CClusterSelect(float(radius), int(min_neighbors), int(min_size), int(keep))
    B.check(fn(_fptr(xyz), n, C.byref(s), _fptr(out), idx.ctypes.data_as(ip), lab.ctypes.data_as(ip), C.byref(m)))
    return out[:m.value].copy(), idx[:m.value].copy(), lab[:m.value].copy()


def cluster_filter(xyz, radius, min_neighbors=0, min_size=0, keep=0):
    """goicp_cluster_filter_host (host only): the points of the `keep` largest clusters (0 = all) with at least `min_size` members, in input
    order -> (cloud (m, 3) float32, their indices (m,) int32, their labels (m,) int32).  Registration.cluster_filter and
    set_source(cluster_radius=, ...) give the same bits on the device."""
    return _cluster_filter_call(B.load_library().goicp_cluster_filter_host, xyz, radius, min_neighbors, min_size, keep)


# goicp_plane, field for field: the planes come back as a structured array
PLANE_DTYPE = np.dtype([("normal", "<f4", (3,)), ("point", "<f4", (3,)), ("d", "<f4"), ("inliers", "<i4"), ("hypothesis", "<i4"), ("refined", "<i4")])


def _plane_select(distance, iterations, refine, max_planes, min_inliers, seed):
    return B.CPlaneSelect(float(distance), int(iterations), int(refine), int(max_planes), int(min_inliers), int(seed) & (2 ** 64 - 1))


def _segment_plane_call(fn, xyz, sel):
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    label, planes, c = np.empty(n, np.int32), np.zeros(B.PLANE_MAX_PLANES, PLANE_DTYPE), C.c_size_t(0)
    B.check(fn(_fptr(xyz), n, C.byref(sel), label.ctypes.data_as(C.POINTER(C.c_int32)), planes.ctypes.data_as(C.POINTER(B.CPlane)), C.byref(c)))
    return label, planes[:c.value].copy()


def segment_plane(xyz, distance, iterations=1000, refine=1, max_planes=1, min_inliers=0, seed=0):
    """goicp_segment_plane_host (host only): RANSAC over `iterations` three-point hypotheses per round, up to `max_planes` rounds, each on
    the points no earlier plane took; a point within `distance` of a plane is its inlier; refine = 1 refits the best hypothesis by least
    squares over its inliers -> (labels (n,) int32, -1 = no plane, planes (c,) PLANE_DTYPE: normal, point, d of normal . x + d = 0, inliers,
    hypothesis, refined).  Registration.segment_plane gives the same bits on the device."""
    return _segment_plane_call(B.load_library().goicp_segment_plane_host, xyz, _plane_select(distance, iterations, refine, max_planes, min_inliers, seed))


def _plane_filter_call(fn, xyz, sel):
    xyz = _f32(xyz, (-1, 3))
    n = len(xyz)
    out, idx, planes, c, m = np.empty((n, 3), np.float32), np.empty(n, np.int32), np.zeros(B.PLANE_MAX_PLANES, PLANE_DTYPE), C.c_size_t(0), C.c_size_t(0)
    B.check(fn(_fptr(xyz), n, C.byref(sel), _fptr(out), idx.ctypes.data_as(C.POINTER(C.c_int32)), planes.ctypes.data_as(C.POINTER(B.CPlane)), C.byref(c),
               C.byref(m)))
    return out[:m.value].copy(), idx[:m.value].copy(), planes[:c.value].copy()


def plane_filter(xyz, distance, iterations=1000, refine=1, max_planes=1, min_inliers=0, seed=0):
    """goicp_plane_filter_host (host only): the points no plane of segment_plane took, in input order -> (cloud (m, 3) float32, their indices
    (m,) int32, planes (c,) PLANE_DTYPE).  Registration.plane_filter and set_source(plane_distance=, ...) give the same bits on the device."""
    return _plane_filter_call(B.load_library().goicp_plane_filter_host, xyz, _plane_select(distance, iterations, refine, max_planes, min_inliers, seed))


# goicp_ransac_pose_result, field for field: the poses come back as a structured array
RANSAC_POSE_DTYPE = np.dtype([("R", "<f4", (3, 3)), ("t", "<f4", (3,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("refined", "<i4")])


def _select_matches_call(index, d2, d2_second, mutual, ratio, require_mutual):
    index, d2, d2_second = np.ascontiguousarray(index, np.int32).reshape(-1), _f32(d2, (-1,)), _f32(d2_second, (-1,))
    nq = len(index)
    if len(d2) != nq or len(d2_second) != nq:
        raise ValueError("select_matches: index, d2 and d2_second must have one entry per query")
    mut = None if mutual is None else np.ascontiguousarray(mutual, np.uint8).reshape(-1)
    if mut is not None and len(mut) != nq:
        raise ValueError("select_matches: one mutual flag per query")
    corr, m = np.empty((nq, 2), np.int32), C.c_size_t(0)
    ip = C.POINTER(C.c_int32)
    B.check(B.load_library().goicp_select_matches(index.ctypes.data_as(ip), _fptr(d2), _fptr(d2_second),
                                                  None if mut is None else mut.ctypes.data_as(C.POINTER(C.c_uint8)), nq, float(ratio),
                                                  int(bool(require_mutual) and mut is not None), corr.ctypes.data_as(ip), C.byref(m)))
    return corr[:m.value].copy()


def select_matches(index, d2, d2_second, mutual=None, ratio=0.0, require_mutual=True):
    """goicp_select_matches (host only): match_features' output -> correspondences (M, 2) int32 (query, target), ascending in the query:
    the queries whose match is mutual (require_mutual; mutual=None: no mutual test) and passes the ratio test d2 <= ratio^2 * d2_second
    (ratio = 0: no ratio test)."""
    return _select_matches_call(index, d2, d2_second, mutual, ratio, require_mutual)


def _ransac_pose_select(distance, iterations, refine, max_poses, min_inliers, edge_similarity, seed):
    return B.CRansacPoseSelect(float(distance), int(iterations), int(refine), int(max_poses), int(min_inliers), float(edge_similarity),
                               int(seed) & (2 ** 64 - 1))


def _ransac_pose_call(fn, src, tgt, corr, sel):
    src, tgt = _f32(src, (-1, 3)), _f32(tgt, (-1, 3))
    corr = np.ascontiguousarray(corr, np.int32).reshape(-1, 2)
    M = len(corr)
    poses, c, mask = np.zeros(B.RANSAC_POSE_MAX_POSES, RANSAC_POSE_DTYPE), C.c_size_t(0), np.zeros(M, np.uint8)
    B.check(fn(_fptr(src), len(src), _fptr(tgt), len(tgt), corr.ctypes.data_as(C.POINTER(C.c_int32)), M, C.byref(sel),
               poses.ctypes.data_as(C.POINTER(B.CRansacPose)), C.byref(c), mask.ctypes.data_as(C.POINTER(C.c_uint8))))
    return poses[:c.value].copy(), mask


def ransac_pose(src, tgt, corr, distance, iterations=100000, refine=1, max_poses=1, min_inliers=0, edge_similarity=0.9, seed=0):
    """goicp_ransac_pose_host (host only): RANSAC over `iterations` three-correspondence hypotheses; a correspondence (source index, target
    index) is an inlier of a pose when |R s + t - m| <= distance; the max_poses best-supported poses with at least max(min_inliers, 3)
    inliers, each refit by least squares over its inliers with refine = 1 -> (poses (c,) RANSAC_POSE_DTYPE: R, t, inliers, hypothesis,
    refined; the inlier mask (M,) uint8 of pose 0).  Registration.ransac_pose gives the same bits on the device."""
    return _ransac_pose_call(B.load_library().goicp_ransac_pose_host, src, tgt, corr,
                             _ransac_pose_select(distance, iterations, refine, max_poses, min_inliers, edge_similarity, seed))


def feature_poses(src, tgt, voxel, k, distance, normal_k=16, viewpoint_src=None, viewpoint_tgt=None, ratio=0.0, require_mutual=True, ops=None, **ransac):
    """voxel_downsample -> estimate_normals -> fpfh -> match_features -> select_matches -> ransac_pose on the host functions (ops: an object
    with the same six methods, a Registration for the device) -> (poses, a dict of the intermediate results: the two downsampled clouds
    'src' / 'tgt', 'corr' and the inlier mask 'inlier').  The poses take the downsampled source onto the downsampled target.  voxel = 0 or
    None: no voxel stage, the clouds as they are."""
    import sys
    o = ops if ops is not None else sys.modules[__name__]
    ds, dt = (o.voxel_downsample(src, voxel)[0], o.voxel_downsample(tgt, voxel)[0]) if voxel else (_f32(src, (-1, 3)), _f32(tgt, (-1, 3)))
    ns, nt = o.estimate_normals(ds, normal_k, viewpoint_src)[0], o.estimate_normals(dt, normal_k, viewpoint_tgt)[0]
    fs, ft = o.fpfh(ds, k, normals=ns)[0], o.fpfh(dt, k, normals=nt)[0]
    idx, d2, second, mut = o.match_features(fs, ft, mutual=True)
    corr = select_matches(idx, d2, second, mut, ratio, require_mutual)
    if len(corr) < 3:
        return np.zeros(0, RANSAC_POSE_DTYPE), {"src": ds, "tgt": dt, "corr": corr, "inlier": np.zeros(len(corr), np.uint8)}
    poses, mask = o.ransac_pose(ds, dt, corr, distance, **ransac)
    return poses, {"src": ds, "tgt": dt, "corr": corr, "inlier": mask}


def _filter_host(pcs, voxel, radius, min_neighbors, stat_neighbors=None, std_ratio=None, cluster=None, plane=None):
    """the composition of the host functions that goicp_set_source_filtered, goicp_set_source_pipeline, goicp_set_source_clustered and
    goicp_set_source_segmented equal"""
    if voxel:
        pcs = voxel_downsample(pcs, voxel)[0]
    if stat_neighbors:
        pcs = statistical_outlier_removal(pcs, stat_neighbors, std_ratio)[0]
    if radius:
        pcs = radius_outlier_removal(pcs, radius, min_neighbors)[0]
    if plane:
        pcs = plane_filter(pcs, *plane)[0]
    if cluster:
        pcs = cluster_filter(pcs, *cluster)[0]
    return pcs


class Config:
    """Config(toml_filepath): same keys, defaults and clamps as the reference; raises on parse error."""

    class _NS:
        pass

    def __init__(self, toml_filepath):
        c = B.CConfig()
        B.check(B.load_library().goicp_config_load(str(toml_filepath).encode(), C.byref(c)))
        self.mode, self.trim = c.mode, bool(c.trim)
        self.subsample, self.mse_threshold, self.resize = c.subsample, c.mse_threshold, c.resize
        self.description = c.description.decode()
        self.io = Config._NS()
        self.io.target, self.io.source = c.target.decode(), c.source.decode()
        self.io.output, self.io.visualization = c.output.decode(), c.visualization.decode()
        self.viz = Config._NS()
        self.viz.theta, self.viz.phi, self.viz.spin_after_finish = c.viz_theta, c.viz_phi, bool(c.viz_spin_after_finish)
        self.rotation = Config._NS()
        self.translation = Config._NS()
        for k, ax in enumerate("xyz"):
            setattr(self.rotation, ax + "min", c.rot_min[k]); setattr(self.rotation, ax + "max", c.rot_max[k])
            setattr(self.translation, ax + "min", c.trans_min[k]); setattr(self.translation, ax + "max", c.trans_max[k])
        self.rotation.search_depth, self.translation.search_depth = c.rot_search_depth, c.trans_search_depth
        self.rotation.present, self.translation.present = bool(c.has_rotation_range), bool(c.has_translation_range)
        self._c = c

    def engine_params(self):
        """Keyword arguments for Registration / FastGoICP carrying what the TOML holds for the engine: the search
        ranges and depths when the [params.rotation] / [params.translation] tables are present."""
        p = B.CParams()
        B.load_library().goicp_params_from_config(C.byref(self._c), C.byref(p))
        out = {}
        if p.use_rot_range:
            out.update(use_rot_range=1, rot_min=list(p.rot_min), rot_max=list(p.rot_max), rot_search_depth=p.rot_search_depth)
        if p.use_trans_range:
            out.update(use_trans_range=1, trans_min=list(p.trans_min), trans_max=list(p.trans_max), trans_search_depth=p.trans_search_depth)
        return out


def load_cloud(filepath, subsample=1.0, resize=1.0, seed=0):
    """load_cloud(path, subsample, resize) -> (n,3) float32.  .ply / .txt; raises GoicpError(GOICP_ERR_IO)."""
    lib = B.load_library()
    p = C.POINTER(C.c_float)()
    n = C.c_size_t(0)
    B.check(lib.goicp_cloud_load(str(filepath).encode(), float(subsample), float(resize), int(seed), C.byref(p), C.byref(n)))
    try:
        out = np.ctypeslib.as_array(p, shape=(n.value * 3,)).copy().reshape(-1, 3) if n.value else np.zeros((0, 3), np.float32)
    finally:
        lib.goicp_cloud_free(p)
    return out


def rodrigues(v):
    v = _f32(v, (3,))
    R = np.empty(9, np.float32)
    B.load_library().goicp_rodrigues(_fptr(v), _fptr(R))
    return R.reshape(3, 3)


class RotNode:
    """Rotation cube in angle-axis space: corner (a,b,c), width w, level l (jly_goicp.h:44-57)."""

    def __init__(self, a, b, c, w, lb=0.0, ub=0.0, l=0):
        self.a, self.b, self.c, self.w, self.lb, self.ub, self.l = map(float, (a, b, c, w, lb, ub, l))
        self.l = int(l)

    @property
    def centre(self):
        h = np.float32(self.w) / np.float32(2)
        return np.array([np.float32(self.a) + h, np.float32(self.b) + h, np.float32(self.c) + h], np.float32)

    @property
    def R(self):
        return rodrigues(self.centre)

    def __lt__(self, o):        # priority order of the reference queues
        return self.lb > o.lb if self.lb != o.lb else self.w < o.w


class TransNode:
    """Translation cube: corner (x,y,z), width w (jly_goicp.h:59-72)."""

    def __init__(self, x, y, z, w, lb=0.0, ub=0.0):
        self.x, self.y, self.z, self.w, self.lb, self.ub = map(float, (x, y, z, w, lb, ub))

    @property
    def centre(self):
        h = np.float32(self.w) / np.float32(2)
        return np.array([np.float32(self.x) + h, np.float32(self.y) + h, np.float32(self.z) + h], np.float32)

    def __lt__(self, o):
        return self.lb > o.lb if self.lb != o.lb else self.w < o.w


class Registration:
    """icp::Registration(pct, nt, pcs, ns): owns the device-resident clouds, DT and k-d tree."""

    def __init__(self, pct, pcs, mse_threshold=1e-3, icp_metric=None, normal_k=None, max_corr_dist=None, robust_kernel=0, robust_scale=0.0, trunc_dist=None,
                 icp_symmetric=False, source_normal_k=16, icp_generalized=False, gicp_epsilon=1e-3, **params):
        """icp_metric / normal_k (not goicp_params fields): goicp_set_icp_options after creation -- 1 makes every ICP of this
        engine point-to-plane (target normals from normal_k neighbours, default 16); None keeps the defaults untouched.
        max_corr_dist: goicp_set_icp_gate after creation -- every ICP of this engine uses only correspondences within that distance.
        robust_kernel / robust_scale: goicp_set_icp_robust after creation -- 1 Huber, 2 Cauchy, 3 Geman-McClure, 4 Tukey (or their names)
        weight every correspondence of every ICP of this engine by its residual; 0 keeps the plain loop.
        trunc_dist: goicp_set_search_truncation after creation -- the search (bounds, pose scores, best_sse) minimises
        sum min(DT(R p + t), trunc_dist)^2 instead of the plain sum of squares; None or 0 keeps the plain objective.
        icp_symmetric / source_normal_k: goicp_set_icp_symmetric after creation -- wherever this engine evaluates metric 1 it takes the
        symmetric point-to-plane form over the normals of both clouds (source normals from source_normal_k neighbours); inert under metric 0.
        icp_generalized / gicp_epsilon: goicp_set_icp_generalized after creation -- wherever this engine evaluates metric 1 it takes the
        generalized (plane-to-plane) form, every correspondence weighted by the combined covariance of both normals; it shares source_normal_k
        with the symmetric flag, the two refuse each other; inert under metric 0."""
        self._lib = B.load_library()
        self.pct, self.pcs = _f32(pct, (-1, 3)), _f32(pcs, (-1, 3))
        p = B.CParams()
        self._lib.goicp_params_default(C.byref(p))
        p.mse_threshold = float(mse_threshold)
        for k, v in params.items():
            if not hasattr(p, k):
                raise TypeError("unknown engine parameter %r" % k)
            if isinstance(getattr(p, k), C.Array):
                v = type(getattr(p, k))(*[float(x) for x in v])
            setattr(p, k, v)
        self.params = p
        h = C.c_void_p()
        B.check(self._lib.goicp_create(C.byref(p), _fptr(self.pct), len(self.pct), _fptr(self.pcs), len(self.pcs), C.byref(h)))
        self.handle = h
        self.ns, self.nt = len(self.pcs), len(self.pct)
        thr, inl = C.c_float(), C.c_int32()
        B.check(self._lib.goicp_thresholds(h, C.byref(thr), C.byref(inl)))
        self.sse_threshold, self.inliers = np.float32(thr.value), inl.value     # as the engine uses them (trimming included)
        if icp_metric is not None or normal_k is not None:
            try:
                self.set_icp_options(0 if icp_metric is None else icp_metric, 16 if normal_k is None else normal_k)
            except Exception:
                self.close()
                raise
        if max_corr_dist is not None:
            try:
                self.set_icp_gate(max_corr_dist)
            except Exception:
                self.close()
                raise

        if robust_kernel:
            try:
                self.set_icp_robust(robust_kernel, robust_scale)
            except Exception:
                self.close()
                raise

        if trunc_dist:
            try:
                self.set_search_truncation(trunc_dist)
            except Exception:
                self.close()
                raise

        if icp_symmetric:
            try:
                self.set_icp_symmetric(True, source_normal_k)
            except Exception:
                self.close()
                raise

        if icp_generalized:
            try:
                self.set_icp_generalized(True, gicp_epsilon, source_normal_k)
            except Exception:
                self.close()
                raise

    # ---- source swap (goicp_set_source) ----
    @property
    def pcs(self):
        """the source cloud in the handle's "original order"; after set_source(voxel=) the reduced cloud, formed on first use (the host
        function's output is the device's, bit for bit, so a scan stream that never asks never pays for a host reduction)"""
        if self._pcs is None:
            self._pcs = _filter_host(*self._pcs_raw)
            self._pcs_raw = None
        return self._pcs

    @pcs.setter
    def pcs(self, value):
        self._pcs, self._pcs_raw = value, None

    def set_source(self, pcs, voxel=None, radius=None, min_neighbors=None, stat_neighbors=None, std_ratio=None, cluster_radius=None,
                   cluster_min_neighbors=0, cluster_min_size=0, cluster_keep=0, plane_distance=None, plane_iterations=0, plane_refine=1, plane_max=1,
                   plane_min_inliers=0, plane_seed=0):
        """goicp_set_source: a new source cloud under the same target.  Everything built from the target, the params and the per-handle
        options stay; afterwards the handle answers as a fresh Registration(pct, pcs, ...) with the same options would, bit for bit.
        voxel: goicp_set_source_voxel -- the cloud is reduced to one centroid per voxel on the device first, and the handle answers as after
        set_source(voxel_downsample(pcs, voxel)[0]); self.ns is the number of points kept, self.pcs the reduced cloud.
        radius, min_neighbors (both or neither): goicp_set_source_filtered -- after the voxel grid, if any, the points with fewer than
        min_neighbors others within radius are dropped on the device, and the handle answers as after set_source of
        radius_outlier_removal(..., radius, min_neighbors)[0].
        stat_neighbors, std_ratio (both or neither): goicp_set_source_pipeline -- between the voxel grid and the radius filter, if any, the
        statistical filter drops the points whose mean distance to their stat_neighbors nearest neighbours is above the mean plus std_ratio
        deviations, and the handle answers as after set_source of the composed host functions' output.
        cluster_radius (with cluster_min_neighbors, cluster_min_size, cluster_keep): goicp_set_source_clustered -- after the other stages, if
        any, only the points of the cluster_keep largest clusters (0 = all) with at least cluster_min_size members stay, and the handle
        answers as after set_source of cluster_filter(..., cluster_radius, cluster_min_neighbors, cluster_min_size, cluster_keep)[0].
        plane_distance (with plane_iterations, plane_refine, plane_max, plane_min_inliers, plane_seed): goicp_set_source_segmented -- between
        the radius filter and the cluster selection, if any, the points of up to plane_max RANSAC planes are dropped, and the handle answers
        as after set_source of plane_filter(..., plane_distance, plane_iterations, ...)[0] followed by the cluster selection."""
        pcs = _f32(pcs, (-1, 3))
        if (radius is None) != (min_neighbors is None):
            raise ValueError("set_source: radius and min_neighbors go together")
        if (stat_neighbors is None) != (std_ratio is None):
            raise ValueError("set_source: stat_neighbors and std_ratio go together")
        if plane_distance is not None:
            if not float(plane_distance) > 0 or (cluster_radius is not None and not float(cluster_radius) > 0) or (voxel is not None and not float(voxel) > 0) \
                    or (radius is not None and not float(radius) > 0) or (stat_neighbors is not None and not int(stat_neighbors) > 0):
                raise ValueError("set_source: a stage that is named needs a size > 0")
            kept = C.c_size_t(0)
            p = B.CSourcePipeline(float(voxel or 0.0), int(stat_neighbors or 0), float(std_ratio or 0.0), float(radius or 0.0), int(min_neighbors or 0))
            plane = (float(plane_distance), int(plane_iterations), int(plane_refine), int(plane_max), int(plane_min_inliers), int(plane_seed))
            cluster = None if cluster_radius is None else (float(cluster_radius), int(cluster_min_neighbors), int(cluster_min_size), int(cluster_keep))
            pl = _plane_select(*plane)
            cs = B.CClusterSelect(*cluster) if cluster else None
            B.check(self._lib.goicp_set_source_segmented(self.handle, _fptr(pcs), len(pcs), C.byref(p), C.byref(pl), C.byref(cs) if cs else None, C.byref(kept)))
            self._pcs, self.ns = None, kept.value
            self._pcs_raw = (pcs, None if voxel is None else float(voxel), None if radius is None else float(radius),
                             None if min_neighbors is None else int(min_neighbors), None if stat_neighbors is None else int(stat_neighbors),
                             None if std_ratio is None else float(std_ratio), cluster, plane)
        elif cluster_radius is not None:
            if not float(cluster_radius) > 0 or (voxel is not None and not float(voxel) > 0) or (radius is not None and not float(radius) > 0) \
                    or (stat_neighbors is not None and not int(stat_neighbors) > 0):
                raise ValueError("set_source: a stage that is named needs a size > 0")
            kept = C.c_size_t(0)
            p = B.CSourcePipeline(float(voxel or 0.0), int(stat_neighbors or 0), float(std_ratio or 0.0), float(radius or 0.0), int(min_neighbors or 0))
            cs = B.CClusterSelect(float(cluster_radius), int(cluster_min_neighbors), int(cluster_min_size), int(cluster_keep))
            B.check(self._lib.goicp_set_source_clustered(self.handle, _fptr(pcs), len(pcs), C.byref(p), C.byref(cs), C.byref(kept)))
            self._pcs, self.ns = None, kept.value
            self._pcs_raw = (pcs, None if voxel is None else float(voxel), None if radius is None else float(radius),
                             None if min_neighbors is None else int(min_neighbors), None if stat_neighbors is None else int(stat_neighbors),
                             None if std_ratio is None else float(std_ratio),
                             (float(cluster_radius), int(cluster_min_neighbors), int(cluster_min_size), int(cluster_keep)))
        elif stat_neighbors is not None:
            if not int(stat_neighbors) > 0 or (voxel is not None and not float(voxel) > 0) or (radius is not None and not float(radius) > 0):
                raise ValueError("set_source: a stage that is named needs a size > 0")
            kept = C.c_size_t(0)
            p = B.CSourcePipeline(float(voxel or 0.0), int(stat_neighbors), float(std_ratio), float(radius or 0.0), int(min_neighbors or 0))
            B.check(self._lib.goicp_set_source_pipeline(self.handle, _fptr(pcs), len(pcs), C.byref(p), C.byref(kept)))
            self._pcs, self.ns = None, kept.value
            self._pcs_raw = (pcs, None if voxel is None else float(voxel), None if radius is None else float(radius),
                             None if min_neighbors is None else int(min_neighbors), int(stat_neighbors), float(std_ratio))
        elif voxel is None and radius is None:
            B.check(self._lib.goicp_set_source(self.handle, _fptr(pcs), len(pcs)))
            self.pcs, self.ns = pcs, len(pcs)
        elif radius is None:
            kept = C.c_size_t(0)
            B.check(self._lib.goicp_set_source_voxel(self.handle, _fptr(pcs), len(pcs), float(voxel), C.byref(kept)))
            self._pcs, self._pcs_raw, self.ns = None, (pcs, float(voxel), None, None), kept.value
        else:
            if not float(radius) > 0 or (voxel is not None and not float(voxel) > 0):
                raise ValueError("set_source: a stage that is named needs a size > 0")
            kept = C.c_size_t(0)
            f = B.CSourceFilter(float(voxel or 0.0), float(radius), int(min_neighbors))
            B.check(self._lib.goicp_set_source_filtered(self.handle, _fptr(pcs), len(pcs), C.byref(f), C.byref(kept)))
            self._pcs, self._pcs_raw, self.ns = None, (pcs, None if voxel is None else float(voxel), float(radius), int(min_neighbors)), kept.value
        thr, inl = C.c_float(), C.c_int32()
        B.check(self._lib.goicp_thresholds(self.handle, C.byref(thr), C.byref(inl)))
        self.sse_threshold, self.inliers = np.float32(thr.value), inl.value

    def voxel_downsample(self, xyz, voxel):
        """goicp_voxel_downsample: the module-level voxel_downsample on the device (the handle lends its device and stream, its state is
        untouched) -> (cloud (m, 3) float32, counts (m,) int32), the same bits"""
        return _voxel_call(lambda *a: self._lib.goicp_voxel_downsample(self.handle, *a), xyz, voxel)

    def radius_outlier_removal(self, xyz, radius, min_neighbors):
        """goicp_radius_outlier_removal: the module-level radius_outlier_removal on the device (the handle lends its device and stream, its
        state is untouched) -> (cloud (m, 3) float32, indices (m,) int32, counts (n,) int32), the same bits"""
        return _outlier_call(lambda *a: self._lib.goicp_radius_outlier_removal(self.handle, *a), xyz, radius, min_neighbors)

    def statistical_outlier_removal(self, xyz, neighbors, std_ratio):
        """goicp_statistical_outlier_removal: the module-level statistical_outlier_removal on the device (the handle lends its device and
        stream, its state is untouched) -> (cloud (m, 3) float32, indices (m,) int32, mean distances (n,) float32, threshold), the same bits"""
        return _stat_call(lambda *a: self._lib.goicp_statistical_outlier_removal(self.handle, *a), xyz, neighbors, std_ratio)

    def cluster(self, xyz, radius, min_neighbors=0):
        """goicp_cluster: the module-level cluster on the device (the handle lends its device and stream, its state is untouched) ->
        (labels (n,) int32, sizes (c,) int32), the same bits"""
        return _cluster_call(lambda *a: self._lib.goicp_cluster(self.handle, *a), xyz, radius, min_neighbors)

    def cluster_filter(self, xyz, radius, min_neighbors=0, min_size=0, keep=0):
        """goicp_cluster_filter: the module-level cluster_filter on the device (the handle lends its device and stream, its state is
        untouched) -> (cloud (m, 3) float32, indices (m,) int32, labels (m,) int32), the same bits"""
        return _cluster_filter_call(lambda *a: self._lib.goicp_cluster_filter(self.handle, *a), xyz, radius, min_neighbors, min_size, keep)

    def segment_plane(self, xyz, distance, iterations=1000, refine=1, max_planes=1, min_inliers=0, seed=0):
        """goicp_segment_plane: the module-level segment_plane on the device (the handle lends its device and stream, its state is
        untouched) -> (labels (n,) int32, planes (c,) PLANE_DTYPE), the same bits"""
        return _segment_plane_call(lambda *a: self._lib.goicp_segment_plane(self.handle, *a), xyz,
                                   _plane_select(distance, iterations, refine, max_planes, min_inliers, seed))

    def plane_filter(self, xyz, distance, iterations=1000, refine=1, max_planes=1, min_inliers=0, seed=0):
        """goicp_plane_filter: the module-level plane_filter on the device (the handle lends its device and stream, its state is
        untouched) -> (cloud (m, 3) float32, indices (m,) int32, planes (c,) PLANE_DTYPE), the same bits"""
        return _plane_filter_call(lambda *a: self._lib.goicp_plane_filter(self.handle, *a), xyz,
                                  _plane_select(distance, iterations, refine, max_planes, min_inliers, seed))

    def knn_self(self, xyz, k):
        """goicp_knn_self: the module-level knn_self on the device (the handle lends its device and stream, its state is untouched)"""
        return _knn_self_call(lambda *a: self._lib.goicp_knn_self(self.handle, *a), xyz, k)

    def estimate_normals(self, xyz, k, viewpoint=None):
        """goicp_estimate_normals: the module-level estimate_normals on the device (the handle lends its device and stream, its state is
        untouched)"""
        return _normals_call(lambda *a: self._lib.goicp_estimate_normals(self.handle, *a), xyz, k, viewpoint)

    def fpfh(self, xyz, k, normals=None, normal_k=16, viewpoint=None):
        """goicp_fpfh: the module-level fpfh on the device, the normals too when none are given (the handle lends its device and stream,
        its state is untouched)"""
        if normals is None:
            normals = self.estimate_normals(xyz, normal_k, viewpoint)[0]
        return _fpfh_call(lambda *a: self._lib.goicp_fpfh(self.handle, *a), xyz, normals, k)

    def match_features(self, fq, ft, mutual=True):
        """goicp_match_features: the module-level match_features on the device (the handle lends its device and stream, its state is
        untouched)"""
        return _match_call(lambda *a: self._lib.goicp_match_features(self.handle, *a), fq, ft, mutual)

    def ransac_pose(self, src, tgt, corr, distance, iterations=100000, refine=1, max_poses=1, min_inliers=0, edge_similarity=0.9, seed=0):
        """goicp_ransac_pose: the module-level ransac_pose on the device (the handle lends its device and stream, its state is untouched)
        -> (poses (c,) RANSAC_POSE_DTYPE, inlier mask (M,) uint8), the same bits"""
        return _ransac_pose_call(lambda *a: self._lib.goicp_ransac_pose(self.handle, *a), src, tgt, corr,
                                 _ransac_pose_select(distance, iterations, refine, max_poses, min_inliers, edge_similarity, seed))

    def feature_poses(self, src, tgt, voxel, k, distance, normal_k=16, viewpoint_src=None, viewpoint_tgt=None, ratio=0.0, require_mutual=True, **ransac):
        """the module-level feature_poses with every stage on the device through this handle (select_matches, linear in the number of
        points, stays on the host) -> (poses, intermediates), the same bits"""
        return feature_poses(src, tgt, voxel, k, distance, normal_k, viewpoint_src, viewpoint_tgt, ratio, require_mutual, ops=self, **ransac)

    def register_features(self, voxel, k, distance, max_iter=10000, err_diff=1e-7, **kw):
        """feature_poses of this handle's own clouds (source onto target; max_poses defaults to 8) as the start poses of icp_run_batch ->
        (R (3, 3), t (3,), err of the candidate with the smallest final error -- the first of equals -- and a dict: 'poses' the start poses,
        'inliers' their counts, 'R' / 't' / 'err' / 'iters' of every candidate after ICP, 'best' the winner's index).  Without a feature
        pose it raises a GoicpError."""
        kw.setdefault("max_poses", 8)
        poses, _ = self.feature_poses(self.pcs, self.pct, voxel, k, distance, **kw)
        if len(poses) == 0:
            raise B.GoicpError(-1, "register_features: the feature matches support no pose")
        R, t, err, it = self.icp_run_batch(poses["R"], poses["t"], max_iter, err_diff)
        best = int(np.argmin(err))
        return R[best], t[best], err[best], {"poses": poses, "inliers": poses["inliers"].copy(), "R": R, "t": t, "err": err, "iters": it, "best": best}

    def debug_source_order(self, xyz, mode=2):
        """goicp_debug_source_order (test): the device ordering alone; equals source_order(xyz, mode)"""
        xyz = _f32(xyz, (-1, 3))
        perm = np.empty(len(xyz), np.int32)
        B.check(self._lib.goicp_debug_source_order(self.handle, _fptr(xyz), len(xyz), int(mode), perm.ctypes.data_as(C.POINTER(C.c_int32))))
        return perm

    # ---- truncated search objective (goicp_set_search_truncation) ----
    def set_search_truncation(self, max_dist=0.0):
        """goicp_set_search_truncation: every term of the search's bounds and scores is clamped at max_dist (0 = off, the plain objective)."""
        B.check(self._lib.goicp_set_search_truncation(self.handle, float(max_dist)))

    def search_truncation(self):
        g = C.c_float()
        B.check(self._lib.goicp_search_truncation(self.handle, C.byref(g)))
        return g.value

    # ---- robust kernel (goicp_icp_robust) ----
    ROBUST_KERNELS = {"none": 0, "huber": 1, "cauchy": 2, "gm": 3, "geman-mcclure": 3, "tukey": 4}

    @staticmethod
    def icp_robust_default():
        r = B.CIcpRobust()
        B.load_library().goicp_icp_robust_default(C.byref(r))
        return r

    def set_icp_robust(self, kernel=0, scale=0.0):
        """goicp_set_icp_robust: kernel 0 off, 1 Huber, 2 Cauchy, 3 Geman-McClure, 4 Tukey (or "huber", "cauchy", "gm", "tukey"); scale c > 0."""
        if isinstance(kernel, str):
            kernel = self.ROBUST_KERNELS[kernel.lower()]
        r = B.CIcpRobust(int(kernel), float(scale))
        B.check(self._lib.goicp_set_icp_robust(self.handle, C.byref(r)))

    def icp_robust_stats(self, K=1):
        """(cost (K,), weight_sum (K,)) of the last pass of the last icp run (K = 1) or icp_run_batch (its K)"""
        c, w = np.empty(int(K), np.float32), np.empty(int(K), np.float32)
        B.check(self._lib.goicp_icp_robust_stats(self.handle, int(K), _fptr(c), _fptr(w)))
        return c, w

    # ---- distance gate (goicp_icp_gate) ----
    @staticmethod
    def icp_gate_default():
        g = B.CIcpGate()
        B.load_library().goicp_icp_gate_default(C.byref(g))
        return g

    def set_icp_gate(self, max_corr_dist=0.0, min_inliers=0, capped_walk=1):
        """goicp_set_icp_gate: a correspondence takes part in an ICP iteration iff its squared distance is <= max_corr_dist^2 (0 = off)."""
        g = B.CIcpGate(float(max_corr_dist), int(min_inliers), int(capped_walk))
        B.check(self._lib.goicp_set_icp_gate(self.handle, C.byref(g)))

    def icp_inliers(self, K=1):
        """inlier counts (K,) of the last icp run (K = 1) or icp_run_batch (its K)"""
        n = np.empty(int(K), np.int32)
        B.check(self._lib.goicp_icp_inliers(self.handle, int(K), n.ctypes.data_as(C.POINTER(C.c_int32))))
        return n

    def eval_correspondences(self, R, t, max_corr_dist=0.0):
        """goicp_eval_correspondences at R|t -> (index (N,) int32, -1 beyond the gate; dist_sq (N,) float32; inliers; sse of the inliers)"""
        R, t = _f32(R, (9,)), _f32(t, (3,))
        idx, d2 = np.empty(self.ns, np.int32), np.empty(self.ns, np.float32)
        n, sse = C.c_int32(), C.c_float()
        B.check(self._lib.goicp_eval_correspondences(self.handle, _fptr(R), _fptr(t), float(max_corr_dist), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     _fptr(d2), C.byref(n), C.byref(sse)))
        return idx, d2, n.value, np.float32(sse.value)

    # ---- pose information (goicp_pose_information) ----
    def pose_information(self, R, t, metric=None, pivot=None, rank_tol=None):
        """goicp_pose_information at R|t -> dict: information (6, 6), gradient, covariance, eigenvalues, eigenvectors (rows), pivot, weight_sum,
        cost, sse, sigma2, inliers, rank, metric, dof_nonpositive.  metric None = the handle's; pivot None = the transformed source centroid."""
        R, t = _f32(R, (9,)), _f32(t, (3,))
        o, out = _pose_info_options(metric, pivot, rank_tol), B.CPoseInfo()
        B.check(self._lib.goicp_pose_information(self.handle, _fptr(R), _fptr(t), C.byref(o), C.byref(out)))
        return _pose_info_dict(out)

    def pose_information_batch(self, R, t, metric=None, pivot=None, rank_tol=None):
        """goicp_pose_information_batch: R (K, 3, 3), t (K, 3) -> list of K dicts, entry k the single call at pose k bit for bit"""
        R, t = _f32(R, (-1, 9)), _f32(t, (-1, 3))
        K = len(R)
        o, out = _pose_info_options(metric, pivot, rank_tol), (B.CPoseInfo * max(K, 1))()
        B.check(self._lib.goicp_pose_information_batch(self.handle, K, _fptr(R), _fptr(t), C.byref(o), out))
        return [_pose_info_dict(out[k]) for k in range(K)]

    def result_information(self, metric=None, pivot=None, rank_tol=None):
        """goicp_result_information: the same at optR | optT of the last finished registration"""
        o, out = _pose_info_options(metric, pivot, rank_tol), B.CPoseInfo()
        B.check(self._lib.goicp_result_information(self.handle, C.byref(o), C.byref(out)))
        return _pose_info_dict(out)

    # ---- ICP metric (goicp_icp_options) ----
    @staticmethod
    def icp_options_default():
        o = B.CIcpOptions()
        B.load_library().goicp_icp_options_default(C.byref(o))
        return o

    def set_icp_options(self, metric=0, normal_k=16):
        """goicp_set_icp_options: 0 point-to-point (default), 1 point-to-plane; builds the target normals for metric 1."""
        o = B.CIcpOptions(int(metric), int(normal_k))
        B.check(self._lib.goicp_set_icp_options(self.handle, C.byref(o)))

    def knn_query(self, q, k):
        """exact k nearest target points -> (index (n, k) int32, dist_sq (n, k) float32), ascending (dist_sq, index)"""
        q = _f32(q, (-1, 3))
        idx, d2 = np.empty((len(q), int(k)), np.int32), np.empty((len(q), int(k)), np.float32)
        B.check(self._lib.goicp_knn_query(self.handle, _fptr(q), len(q), int(k), idx.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(d2)))
        return idx, d2

    def target_normals(self):
        """(M, 3) float32 target normals in the target's order (built on first use)"""
        n = np.empty((self.nt, 3), np.float32)
        B.check(self._lib.goicp_target_normals(self.handle, _fptr(n)))
        return n

    # ---- symmetric point-to-plane ICP (goicp_set_icp_symmetric) ----
    def set_icp_symmetric(self, enabled=True, source_normal_k=16):
        """goicp_set_icp_symmetric: metric 1 in its symmetric form over the normals of both clouds; stored and inert under metric 0."""
        B.check(self._lib.goicp_set_icp_symmetric(self.handle, int(bool(enabled)), int(source_normal_k)))

    def icp_symmetric(self):
        """goicp_get_icp_symmetric -> (enabled, source_normal_k, user_normals)"""
        e, k, u = C.c_int32(), C.c_int32(), C.c_int32()
        B.check(self._lib.goicp_get_icp_symmetric(self.handle, C.byref(e), C.byref(k), C.byref(u)))
        return bool(e.value), k.value, bool(u.value)

    # ---- generalized (plane-to-plane) ICP (goicp_set_icp_generalized) ----
    def set_icp_generalized(self, enabled=True, epsilon=1e-3, source_normal_k=16):
        """goicp_set_icp_generalized: metric 1 in its generalized form, W = 2 eps (C_m + R C_p R^T)^-1 from the normals of both clouds; stored
        and inert under metric 0."""
        B.check(self._lib.goicp_set_icp_generalized(self.handle, int(bool(enabled)), float(epsilon), int(source_normal_k)))

    def get_icp_generalized(self):
        """goicp_get_icp_generalized -> (enabled, epsilon, source_normal_k, user_normals)"""
        e, eps, k, u = C.c_int32(), C.c_float(), C.c_int32(), C.c_int32()
        B.check(self._lib.goicp_get_icp_generalized(self.handle, C.byref(e), C.byref(eps), C.byref(k), C.byref(u)))
        return bool(e.value), eps.value, k.value, bool(u.value)

    def source_normals(self):
        """(N, 3) float32 source normals in the source's original order: the estimated ones (built on first use) or the caller's"""
        n = np.empty((self.ns, 3), np.float32)
        B.check(self._lib.goicp_source_normals(self.handle, _fptr(n)))
        return n

    def set_source_normals(self, normals):
        """goicp_set_source_normals: the caller's normals (N x 3, original source order, each zero or of unit length) until the next swap"""
        normals = _f32(normals, (-1, 3))
        B.check(self._lib.goicp_set_source_normals(self.handle, _fptr(normals), len(normals)))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.goicp_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- DT ----
    def dt_info(self):
        V, s, o = C.c_int32(), C.c_double(), (C.c_double * 3)()
        B.check(self._lib.goicp_dt_info(self.handle, C.byref(V), C.byref(s), o))
        return V.value, s.value, tuple(o)

    def dt_download(self):
        V = self.dt_info()[0]
        g = np.empty(V ** 3, np.float32)
        B.check(self._lib.goicp_dt_download(self.handle, _fptr(g)))
        return g.reshape(V, V, V)

    def rot_coeff(self, level):
        return np.float32(self._lib.goicp_rot_coeff(self.handle, int(level)))

    # ---- the two compute_sse_error overloads ----
    def compute_sse_error(self, *args, **kw):
        """compute_sse_error(R, t) -> sse   |   compute_sse_error(rnode, tnodes, fix_rot) -> (lb[], ub[])"""
        if len(args) >= 2 and isinstance(args[0], RotNode):
            rnode, tnodes = args[0], args[1]
            fix_rot = args[2] if len(args) > 2 else kw.get("fix_rot", True)
            cubes = np.array([[*t.centre, np.float32(t.w)] for t in tnodes], np.float32).reshape(-1, 4)
            ub, lb = self.eval_bounds(rnode.R, cubes, -1 if fix_rot else rnode.l)
            return lb, ub
        R, t = _f32(args[0], (9,)), _f32(args[1], (3,))
        sse = C.c_float()
        B.check(self._lib.goicp_eval_sse(self.handle, _fptr(R), _fptr(t), C.byref(sse)))
        return np.float32(sse.value)

    def eval_bounds(self, R, cubes, level=-1):
        R, cubes = _f32(R, (9,)), _f32(cubes, (-1, 4))
        n = len(cubes)
        ub, lb = np.empty(n, np.float32), np.empty(n, np.float32)
        B.check(self._lib.goicp_eval_bounds(self.handle, _fptr(R), _fptr(cubes), n, int(level), _fptr(ub), _fptr(lb)))
        return ub, lb

    def eval_bounds_batch(self, rots, cubes):
        """rots (K,3,3); cubes structured array of binding.CCube (or (B,6) with rot in the last col)."""
        rots = _f32(rots, (-1, 9))
        arr = (B.CCube * len(cubes))(*[B.CCube(*map(float, c[:5]), int(c[5])) for c in cubes])
        n = len(cubes)
        ub, lb = np.empty(n, np.float32), np.empty(n, np.float32)
        B.check(self._lib.goicp_eval_bounds_batch(self.handle, _fptr(rots), len(rots), arr, n, _fptr(ub), _fptr(lb)))
        return ub, lb

    def inner_bnb(self, R, level=-1, incumbent=1e10):
        """branch_and_bound_R3(rnode, fix_rot): -> (value, best_node[4] or None, counters)"""
        R = _f32(R, (9,))
        val, node, cnt = C.c_float(), np.full(4, np.nan, np.float32), B.CCounters()
        B.check(self._lib.goicp_inner_bnb(self.handle, _fptr(R), int(level), float(incumbent), C.byref(val), _fptr(node), C.byref(cnt)))
        return np.float32(val.value), (None if np.isnan(node[3]) else node), cnt

    def nn_query(self, q):
        q = _f32(q, (-1, 3))
        idx, d2 = np.empty(len(q), np.int32), np.empty(len(q), np.float32)
        B.check(self._lib.goicp_nn_query(self.handle, _fptr(q), len(q), idx.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(d2)))
        return idx, d2

    def transform_source(self, R, t):
        R, t = _f32(R, (9,)), _f32(t, (3,))
        out = np.empty((self.ns, 3), np.float32)
        B.check(self._lib.goicp_transform_source(self.handle, _fptr(R), _fptr(t), _fptr(out)))
        return out

    def icp_step(self):
        B.check(self._lib.goicp_icp_step(self.handle))
        return self.poll()

    def icp_run_batch(self, R, t, max_iter=10000, err_diff=1e-7):
        """goicp_icp_run_batch: K independent ICP runs (this handle's ICP options), one per start pose, refined together on the device.
        R (K,3,3) or (K,9), t (K,3) -> (R (K,3,3), t (K,3), err (K,), iters (K,)); pose k is bit for bit the single run from R[k], t[k]."""
        R, t = np.asarray(R), np.asarray(t)
        if R.ndim not in (2, 3) or R.shape[1:] not in ((3, 3), (9,)) or t.ndim != 2 or t.shape[1] != 3 or len(R) != len(t) or len(R) == 0:
            raise ValueError("icp_run_batch: R must be (K,3,3) or (K,9) and t (K,3) with the same K >= 1, got %s and %s" % (R.shape, t.shape))
        K = len(R)
        R, t = _f32(R, (K, 9)).copy(), _f32(t, (K, 3)).copy()
        err, it = np.empty(K, np.float32), np.empty(K, np.int32)
        B.check(self._lib.goicp_icp_run_batch(self.handle, K, _fptr(R), _fptr(t), int(max_iter), float(err_diff), _fptr(err),
                                              it.ctypes.data_as(C.POINTER(C.c_int32))))
        return R.reshape(K, 3, 3), t, err, it

    def icp_run_collective(self, comm_ops, R=None, t=None, max_iter=10000, err_diff=1e-7, raise_on_error=True):
        """goicp_icp_run_collective: ICP3D::Run with the source points sharded over the ranks of comm_ops (a binding.CCommOps); every rank
        calls it with the same arguments and gets the world-1 result bit for bit.  -> (status, err, R (3,3), t, iters)"""
        R = _f32(np.eye(3) if R is None else R, (9,)).copy()
        t = _f32(np.zeros(3) if t is None else t, (3,)).copy()
        err, it = C.c_float(), C.c_int32()
        rc = self._lib.goicp_icp_run_collective(self.handle, C.byref(comm_ops), _fptr(R), _fptr(t), int(max_iter), float(err_diff),
                                                C.byref(err), C.byref(it))
        if raise_on_error:
            B.check(rc)
        return rc, np.float32(err.value), R.reshape(3, 3), t, it.value

    def icp_shard_stats(self):
        """goicp_icp_shard_stats_get as a dict: this engine's collective ICP runs since it was created."""
        st = B.CIcpShardStats()
        B.check(self._lib.goicp_icp_shard_stats_get(self.handle, C.byref(st)))
        return {k: getattr(st, k) for k, _ in B.CIcpShardStats._fields_}

    def poll(self):
        r = B.CResult()
        B.check(self._lib.goicp_poll(self.handle, C.byref(r)))
        return r


class IterativeClosestPoint3D:
    """IterativeClosestPoint3D(reg, pct, pcs, max_iter, threshold, R, t).run() -> (sse, R, t).
    `threshold` is the reference CPU path's err_diff (mean squared error decrease per point)."""

    def __init__(self, reg, max_iter=10000, convergence_threshold=1e-7, R=None, t=None, icp_metric=None, normal_k=None, max_corr_dist=None):
        self.reg, self.max_iter, self.thr = reg, int(max_iter), float(convergence_threshold)
        if max_corr_dist is not None:                           # the gate of reg's handle (every ICP it runs)
            reg.set_icp_gate(max_corr_dist)
        if icp_metric is not None or normal_k is not None:      # the options of reg's handle (every ICP it runs)
            reg.set_icp_options(0 if icp_metric is None else icp_metric, 16 if normal_k is None else normal_k)
        self.R = _f32(np.eye(3) if R is None else R, (9,)).copy()
        self.t = _f32(np.zeros(3) if t is None else t, (3,)).copy()
        self.iters = 0

    def run(self):
        err, it = C.c_float(), C.c_int32()
        B.check(self.reg._lib.goicp_icp_run(self.reg.handle, _fptr(self.R), _fptr(self.t), self.max_iter, self.thr,
                                            C.byref(err), C.byref(it)))
        self.iters = it.value
        return np.float32(err.value), self.R.reshape(3, 3).copy(), self.t.copy()


class FastGoICP:
    """icp::FastGoICP(pct, pcs, mse_threshold, mtx): run() blocks (use a worker thread), the result
    fields are a consistent snapshot (the reference published them unlocked)."""

    def __init__(self, pct, pcs, mse_threshold, mtx=None, icp_metric=None, normal_k=None, max_corr_dist=None, trunc_dist=None, **params):
        # icp_symmetric / icp_generalized / gicp_epsilon / source_normal_k and the goicp_params fields travel in **params
        self.registration = Registration(pct, pcs, mse_threshold, icp_metric=icp_metric, normal_k=normal_k, max_corr_dist=max_corr_dist,
                                         trunc_dist=trunc_dist, **params)
        self.mtx = mtx or threading.Lock()
        self.mse_threshold = float(mse_threshold)
        self.sse_threshold = self.registration.sse_threshold      # mse_threshold * inlierNum (jly_goicp.cpp:198-208), from the engine

    def set_source(self, pcs, voxel=None, radius=None, min_neighbors=None, stat_neighbors=None, std_ratio=None, cluster_radius=None,
                   cluster_min_neighbors=0, cluster_min_size=0, cluster_keep=0, plane_distance=None, plane_iterations=0, plane_refine=1, plane_max=1,
                   plane_min_inliers=0, plane_seed=0):
        """Registration.set_source, then the fields this object mirrors are read again (the polled snapshot is the fresh handle's)"""
        self.registration.set_source(pcs, voxel, radius, min_neighbors, stat_neighbors, std_ratio, cluster_radius, cluster_min_neighbors,
                                     cluster_min_size, cluster_keep, plane_distance, plane_iterations, plane_refine, plane_max, plane_min_inliers,
                                     plane_seed)
        self.sse_threshold = self.registration.sse_threshold

    def run(self):
        B.check(self.registration._lib.goicp_register(self.registration.handle))

    def cancel(self):
        B.check(self.registration._lib.goicp_cancel(self.registration.handle))

    def _snap(self):
        return self.registration.poll()

    def get_best_error(self):
        return np.float32(self._snap().best_sse)

    optR = property(lambda s: np.array(s._snap().optR, np.float32).reshape(3, 3))
    optT = property(lambda s: np.array(s._snap().optT, np.float32))
    curR = property(lambda s: np.array(s._snap().curR, np.float32).reshape(3, 3))
    curT = property(lambda s: np.array(s._snap().curT, np.float32))
    finished = property(lambda s: bool(s._snap().finished))
    counters = property(lambda s: s._snap().counters)

    def information(self, metric=None, pivot=None, rank_tol=None):
        """information matrix, covariance and rank at the registration's result (Registration.result_information)"""
        return self.registration.result_information(metric, pivot, rank_tol)

    def write_output(self, path):
        B.check(self.registration._lib.goicp_result_write_toml(self.registration.handle, str(path).encode()))

    def write_visualization(self, path):
        B.check(self.registration._lib.goicp_result_write_ply(self.registration.handle, str(path).encode()))

    # stepped API used by the sharded driver
    def set_shard(self, rank, world):
        B.check(self.registration._lib.goicp_set_shard(self.registration.handle, rank, world))

    def register_begin(self):
        B.check(self.registration._lib.goicp_register_begin(self.registration.handle))

    def register_step(self, max_rot_pops=8):
        s = B.CStepStatus()
        B.check(self.registration._lib.goicp_register_step(self.registration.handle, int(max_rot_pops), C.byref(s)))
        return {"finished": bool(s.finished), "early_exit": bool(s.early_exit), "best_sse": float(s.best_sse),
                "frontier_lb": float(s.frontier_lb), "rot_pops": int(s.rot_pops)}

    def offer_best(self, sse, R, t):
        R, t = _f32(R, (9,)), _f32(t, (3,))
        B.check(self.registration._lib.goicp_offer_best(self.registration.handle, float(sse), _fptr(R), _fptr(t)))

    def register_end(self):
        B.check(self.registration._lib.goicp_register_end(self.registration.handle))

    def pose(self):
        r = self._snap()
        return float(r.best_sse), np.array(r.optR, np.float32), np.array(r.optT, np.float32)
