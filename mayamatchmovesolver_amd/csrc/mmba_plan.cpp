// mmba_plan.cpp -- plan construction: validation, parameter classification,
// observation ordering and the symbolic structure of the reduced system.
//
// The classification replaces the dense errorToParamList / paramFrameList of
// the reference (adjust_relationships.cpp:565-617, :270-329): every
// parameter is one of
//   CF  animated attribute that only reaches one camera at one frame
//       (camera pose, focal per frame)          -> camera-frame block
//   B   static attribute that only reaches one bundle
//       (bundle translate)                      -> bundle block (Schur)
//   G   anything else (static camera attrs, lens coefficients, group
//       transforms shared by several bundles/cameras) -> dense arrow rows
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <unordered_map>
#include <numeric>
#include <set>

#include "mmba_kernels.h"
#include "mmba_plan.h"

namespace mmba {

Plan::~Plan() {
    if (d_k2probe) {
        // the last k_jac_ne_u launch: per workgroup entry / staged / observations
        // done / exit (10-ns ticks), summarised in microseconds
        // the tail in its parts: the wave sums up to their barrier, the
        // Acc / g stores up to the epilogue, the epilogue
        constexpr int N = K2_PROBE_N;
        std::vector<long long> t(N * (size_t)ncf);
        if (hipMemcpy(t.data(), d_k2probe, sizeof(long long) * t.size(), hipMemcpyDeviceToHost) ==
            hipSuccess) {
            long long t0 = LLONG_MAX, tend = 0;
            for (int c = 0; c < ncf; ++c)
                if (t[N * c]) {
                    t0 = std::min(t0, t[N * c]);
                    tend = std::max(tend, t[N * c + 3]);
                }
            std::vector<double> st, stg, obs, tail, tot, sums, stor, epi;
            int per_xcc[16] = {};
            for (int c = 0; c < ncf; ++c) {
                const long long *q = &t[N * c];
                if (!q[0]) continue;
                st.push_back((q[0] - t0) / 100.);
                stg.push_back((q[1] - q[0]) / 100.);
                obs.push_back((q[2] - q[1]) / 100.);
                tail.push_back((q[3] - q[2]) / 100.);
                tot.push_back((q[3] - q[0]) / 100.);
                per_xcc[q[4] & 15]++;
                if (q[6] && q[7]) {
                    sums.push_back((q[6] - q[2]) / 100.);
                    stor.push_back((q[7] - q[6]) / 100.);
                    epi.push_back((q[3] - q[7]) / 100.);
                }
            }
            auto pct = [](std::vector<double> v, double p) {
                if (v.empty()) return 0.;
                std::sort(v.begin(), v.end());
                return v[std::min(v.size() - 1, (size_t)(p * (v.size() - 1) + 0.5))];
            };
            std::fprintf(stderr, "[mmba probe] k_jac_ne_u %zu workgroups, span %.2f us; p0/p50/p100 "
                                 "(us): start %.2f/%.2f/%.2f staging %.2f/%.2f/%.2f observations "
                                 "%.2f/%.2f/%.2f tail %.2f/%.2f/%.2f total %.2f/%.2f/%.2f; per XCC",
                         st.size(), (tend - t0) / 100., pct(st, 0), pct(st, .5), pct(st, 1),
                         pct(stg, 0), pct(stg, .5), pct(stg, 1), pct(obs, 0), pct(obs, .5),
                         pct(obs, 1), pct(tail, 0), pct(tail, .5), pct(tail, 1), pct(tot, 0),
                         pct(tot, .5), pct(tot, 1));
            for (int x = 0; x < 8; ++x) std::fprintf(stderr, " %d", per_xcc[x]);
            std::fprintf(stderr, "; tail: sums %.2f/%.2f/%.2f stores %.2f/%.2f/%.2f "
                                 "epilogue %.2f/%.2f/%.2f\n",
                         pct(sums, 0), pct(sums, .5), pct(sums, 1), pct(stor, 0), pct(stor, .5),
                         pct(stor, 1), pct(epi, 0), pct(epi, .5), pct(epi, 1));
        }
    }
    if (d_probe && bs.use_bcr && bs.bcr.fflags && bs.bcr.nblk >= 2) {
        // dataflow factor trace of the last factorisation: per level, the
        // mean wait, item and publish times and the level's span (us)
        const int nit = bs.bcr.nblk + 64;
        std::vector<long long> t((size_t)8 + 4 * nit, 0);
        if (hipMemcpy(t.data(), d_probe, sizeof(long long) * t.size(), hipMemcpyDeviceToHost) ==
            hipSuccess) {
            std::fprintf(stderr,
                         "[mmba probe] bcr df phase 10-ns ticks (workgroup 0, all items, all solves): "
                         "stage %lld a-load %lld chain %lld store %lld mfma-upd %lld tail %lld\n",
                         t[0], t[1], t[2], t[3], t[4], t[5]);
            const long long *tr = t.data() + 8;
            long long t0 = tr[0];
            for (int i = 0; i < nit && (tr[4 * i] || tr[4 * i + 3]); ++i) t0 = std::min(t0, tr[4 * i]);
            int base = 0, lvl = 0;
            for (int nact = bs.bcr.nblk;; nact = (nact + 1) / 2, ++lvl) {
                const int g = nact > 1 ? (nact + 1) / 2 : 1;
                double w = 0, c = 0, p = 0, lo = 1e30, hi = 0;
                for (int i = base; i < base + g; ++i) {
                    const long long *q = tr + 4 * i;
                    w += q[1] - q[0];
                    c += q[2] - q[1];
                    p += q[3] - q[2];
                    lo = std::min(lo, (double)(q[1] - t0));
                    hi = std::max(hi, (double)(q[3] - t0));
                }
                std::fprintf(stderr,
                             "[mmba probe] bcr df level %d items %d: wait %.2f item %.2f publish "
                             "%.2f us (means); work from %.2f to %.2f us\n",
                             lvl, g, w / g / 100., c / g / 100., p / g / 100., lo / 100.,
                             hi / 100.);
                base += g;
                if (nact <= 1) break;
            }
        }
    } else if (d_probe && bs.use_bcr) {
        long long h[6] = {0, 0, 0, 0, 0, 0};
        if (hipMemcpy(h, d_probe, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
            std::fprintf(stderr,
                         "[mmba probe] bcr level 10-ns ticks (workgroup 0, all levels): stage %lld "
                         "a-load %lld chain %lld store %lld mfma-upd %lld tail %lld (K=%d nblk=%d)\n",
                         h[0], h[1], h[2], h[3], h[4], h[5], bs.bcr.K, bs.bcr.nblk);
    } else if (d_probe) {
        long long h[4] = {0, 0, 0, 0};
        if (hipMemcpy(h, d_probe, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
            std::fprintf(stderr,
                         "[mmba probe] band factor cycles (partition 0): diag+move %lld panel %lld "
                         "update %lld tail %lld (nb=%d w=%d nG=%d P=%d)\n",
                         h[0], h[1], h[2], h[3], nR - nG, bw, nG, bs.P);
    }
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    if (ev_sync) (void)hipEventDestroy(ev_sync);
    if (hb_pending)
        for (hipStream_t c : s_hb)
            if (c) (void)hipStreamSynchronize(c);
    for (hipEvent_t e : ev_hb)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t c : s_hb)
        if (c) (void)hipStreamDestroy(c);
    for (void *p : allocs) (void)hipFree(p);
    if (h_scalar) (void)hipHostFree(h_scalar);
    if (h_fail) (void)hipHostFree(h_fail);
    if (h_bflag) (void)hipHostFree(h_bflag);
    if (h_xstage) (void)hipHostFree(h_xstage);
    if (h_seq) (void)hipHostFree(h_seq);
    if (h_pack) (void)hipHostFree(h_pack);
    if (h_met) (void)hipHostFree(h_met);
    if (h_mk) (void)hipHostFree(h_mk);
}

static void require(bool c, const char *what) {
    if (!c) throw Invalid{what};
}

// Frame partition of a sharded solve, shared with the host-only
// ABI entry mmba_shard_layout: shard k owns frames [bounds[k], bounds[k+1]),
// the first frame whose cumulative observation count reaches k * M / nranks
// starting shard k; a bundle belongs to the shard holding its first
// (earliest-frame) observation.
void shard_layout(int F, int M, const int32_t *obs_frame, const int32_t *obs_bnd, int nB,
                  int nranks, int32_t *bounds, int32_t *bnd_owner) {
    std::vector<long long> per_frame(F + 1, 0);
    for (int i = 0; i < M; ++i) per_frame[obs_frame[i] + 1]++;
    for (int f = 0; f < F; ++f) per_frame[f + 1] += per_frame[f];
    for (int k = 0; k <= nranks; ++k) bounds[k] = F;
    bounds[0] = 0;
    for (int k = 1; k < nranks; ++k) {
        const long long target = (long long)k * M / nranks;
        int f = bounds[k - 1];
        while (f < F && per_frame[f] < target) ++f;
        bounds[k] = f;
    }
    if (!bnd_owner) return;
    std::vector<int> bnd_first(nB, F);
    for (int i = 0; i < M; ++i)
        bnd_first[obs_bnd[i]] = std::min(bnd_first[obs_bnd[i]], (int)obs_frame[i]);
    for (int b = 0; b < nB; ++b) {
        int k = 0;
        while (k + 1 < nranks && bounds[k + 1] <= bnd_first[b]) ++k;
        bnd_owner[b] = k;
    }
}

thread_local bool t_lens_plain = false;
thread_local bool t_obj_cf = false;

// Lens instances (mmba.h ABI 7; oracle/refcpu.c b3_build
// is the checker's restatement).  The reference clones every lens model once
// per frame, instance (l, f), and reads its lookup lists at mixed indices:
// observation (marker i, frame f) is distorted by instance
// (lens of marker (i + f) / F, (i + f) % F) (adjust_measureErrors.cpp:244,
// 463 on the list of maya_lens_model_utils.cpp:782-799), and setParameters
// writes attrList entry a's value at frame g into instance (lens of entry
// (a + g) / F, (a + g) % F) -- every g for a static attribute
// (adjust_setParameters.cpp:113-121, 206-214; list :836-851), skipping
// entries without a lens, the last parameter winning.  A slot no parameter
// writes holds the plug model's value.  Only the instances some observation
// reads are kept.  With t_lens_plain (the per-frame solves, where the
// reference's frame list has one frame and no index mixes) every
// observation reads its own camera's lens at its own frame and every
// parameter writes its own lens.
void Plan::build_lens_instances(const mmba_problem *pr) {
    const int nL = pr->num_lenses, nK = pr->num_markers;
    obs_inst_g.assign(Mg, -1);
    inst_lens_h.clear();
    inst_attr_h.clear();
    inst_frame_h.clear();
    inst_val_h.clear();
    inst_lpar_off_h.assign(1, 0);
    inst_lpar_h.clear();
    if (!pr->cam_lens || nL <= 0) return;
    const bool plain = t_lens_plain;
    auto lens_of_marker = [&](int i) { return pr->cam_lens[pr->mkr_cam[i]]; };
    std::unordered_map<long long, int> inst_id;
    for (int r = 0; r < Mg; ++r) {
        const long long t = (long long)pr->obs_marker[r] + pr->obs_frame[r];
        const int owner = plain ? pr->obs_marker[r] : (int)(t / F);
        const int f = plain ? pr->obs_frame[r] : (int)(t % F);
        require(owner < nK, "marker index + frame index past the marker list (B3)");
        const int l = lens_of_marker(owner);
        if (l < 0) continue;
        const long long key = (long long)l * F + f;
        auto it = inst_id.find(key);
        if (it == inst_id.end()) {
            const int id = (int)inst_lens_h.size();
            it = inst_id.emplace(key, id).first;
            inst_lens_h.push_back(l);
            const int type = pr->lens_type[l];
            const bool classic = type == MMBA_LENS_3DE_CLASSIC;
            const bool anam = type == MMBA_LENS_3DE_ANAMORPHIC_STD_DEG4 ||
                              type == MMBA_LENS_3DE_ANAMORPHIC_STD_DEG4_RESCALED;
            for (int k = 0; k < MMBA_LENS_NUM_ATTRS; ++k) {
                // the plug model's value (lens attributes are never read per
                // frame, B11): lens_input_values, or the attribute at frame 0
                double v = ((classic && k == 1) || (anam && k >= 11)) ? 1. : 0.;
                const int a = pr->lens_attrs[MMBA_LENS_NUM_ATTRS * l + k];
                if (pr->lens_input_values) v = pr->lens_input_values[(size_t)MMBA_LENS_NUM_ATTRS * l + k];
                else if (a >= 0) v = pr->attr_values[pr->attr_offset[a]];
                inst_attr_h.push_back(-1);
                inst_frame_h.push_back(0);
                inst_val_h.push_back(v);
            }
        }
        obs_inst_g[r] = it->second;
    }
    const int ninst = (int)inst_lens_h.size();
    // (lens, slot) of each attribute id
    std::unordered_map<int, std::pair<int, int>> lens_slot;
    for (int l = nL - 1; l >= 0; --l)
        for (int k = MMBA_LENS_NUM_ATTRS - 1; k >= 0; --k) {
            const int a = pr->lens_attrs[MMBA_LENS_NUM_ATTRS * l + k];
            if (a >= 0) lens_slot[a] = {l, k};
        }
    // attrList indices: param_ref_attr, or numbered by first appearance
    std::vector<int> par_ref(n);
    int n_ref = 0;
    if (pr->param_ref_attr) {
        n_ref = pr->num_ref_attrs;
        for (int p = 0; p < n; ++p) par_ref[p] = pr->param_ref_attr[p];
    } else {
        std::unordered_map<int, int> first;
        for (int p = 0; p < n; ++p) {
            auto it = first.find(pr->param_attr[p]);
            if (it == first.end()) it = first.emplace(pr->param_attr[p], n_ref++).first;
            par_ref[p] = it->second;
        }
    }
    std::vector<int> ref_lens(std::max(n_ref, 1), -1);
    if (pr->ref_attr_lens) {
        for (int r = 0; r < n_ref; ++r) ref_lens[r] = pr->ref_attr_lens[r];
    } else {
        for (int p = n - 1; p >= 0; --p) {
            auto it = lens_slot.find(pr->param_attr[p]);
            if (par_ref[p] >= 0 && par_ref[p] < n_ref)
                ref_lens[par_ref[p]] = it == lens_slot.end() ? -1 : it->second.first;
        }
    }
    for (int r = 0; r < n_ref; ++r) require(ref_lens[r] < nL, "ref_attr_lens");
    // setParameters' lens writes, in parameter order (the last one stays)
    std::vector<int> src((size_t)ninst * MMBA_LENS_NUM_ATTRS, -1);
    for (int p = 0; p < n; ++p) {
        auto ls = lens_slot.find(pr->param_attr[p]);
        if (ls == lens_slot.end()) continue;
        const int la = ls->second.first, k = ls->second.second;
        const int g0 = pr->param_frame[p] >= 0 ? pr->param_frame[p] : 0;
        const int g1 = pr->param_frame[p] >= 0 ? pr->param_frame[p] + 1 : F;
        require(par_ref[p] >= 0 && par_ref[p] < n_ref, "param_ref_attr");
        for (int g = g0; g < g1; ++g) {
            const long long t = (long long)par_ref[p] + g;
            const int lt = plain ? la : ref_lens[t / F];
            const int f = plain ? g : (int)(t % F);
            if (lt < 0) continue;  // a null model: setLensModelAttributeValue ignores it
            if (pr->lens_type[lt] != pr->lens_type[la])
                throw Unsupported{"a lens attribute written into a lens of another model "
                                  "type (B3: undefined in the reference)"};
            auto it = inst_id.find((long long)lt * F + f);
            if (it != inst_id.end()) src[(size_t)it->second * MMBA_LENS_NUM_ATTRS + k] = p;
        }
    }
    for (int j = 0; j < ninst; ++j) {
        std::vector<int> ps;
        for (int k = 0; k < MMBA_LENS_NUM_ATTRS; ++k) {
            const int p = src[(size_t)j * MMBA_LENS_NUM_ATTRS + k];
            if (p < 0) continue;
            inst_attr_h[(size_t)j * MMBA_LENS_NUM_ATTRS + k] = pr->param_attr[p];
            inst_frame_h[(size_t)j * MMBA_LENS_NUM_ATTRS + k] =
                pr->param_frame[p] >= 0 ? pr->param_frame[p] : 0;
            ps.push_back(p);
        }
        std::sort(ps.begin(), ps.end());
        for (int p : ps) inst_lpar_h.push_back(p);
        inst_lpar_off_h.push_back((int)inst_lpar_h.size());
    }
}

void Plan::build(const mmba_problem *pr, const mmba_options *o) {
    require(pr && o, "null problem/options");
    opt = *o;
    s = ctx->stream;
    F = pr->num_frames;
    const int nA = pr->num_attrs, nT = pr->num_transforms, nC = pr->num_cameras;
    const int nL = pr->num_lenses, nK = pr->num_markers;
    nB = pr->num_bundles;
    Mg = pr->num_obs;
    nrows = (pr->num_stiff > 0 ? pr->num_stiff : 0) + (pr->num_smooth > 0 ? pr->num_smooth : 0);
    mg = 2 * Mg + nrows;
    M = Mg;  // local observations: all of them unless sharded (below)
    n = pr->num_params;
    m = 2 * M + nrows;
    rank = comm && !replicated ? comm->rank : 0;
    nranks = comm && !replicated ? comm->nranks : 1;
    require(F > 0 && M > 0 && n > 0, "empty problem");
    require(n <= m, "more parameters than errors (adjust_base.cpp:864)");
    require(opt.solver_type == MMBA_SOLVER_CMINPACK_LMDER ||
                opt.solver_type == MMBA_SOLVER_CMINPACK_LMDIF,
            "solver_type");
    require(opt.scene_graph_mode == MMBA_SCENE_GRAPH_MAYA_DAG ||
                opt.scene_graph_mode == MMBA_SCENE_GRAPH_MM_SCENE_GRAPH,
            "scene_graph_mode");
    const bool lmder_opt = opt.solver_type == MMBA_SOLVER_CMINPACK_LMDER;
    // lmdif never reads autoDiffType (its fdjac2 is always forward)
    central = lmder_opt && opt.auto_diff_type == MMBA_AUTO_DIFF_CENTRAL;
    if (opt.robust_loss)
        require(opt.robust_loss_type >= MMBA_ROBUST_LOSS_TRIVIAL &&
                    opt.robust_loss_type <= MMBA_ROBUST_LOSS_CAUCHY && opt.robust_loss_scale != 0.,
                "robust_loss_type / robust_loss_scale");

    // rolling shutter (mmba.h ABI 3, mmba_rs.hip): on when some camera has
    // rs != 0 and there is more than one frame (oracle/refcpu.c rs_on)
    rs_on = false;
    if (pr->cam_rs_value && F > 1)
        for (int c = 0; c < pr->num_cameras; ++c)
            if (pr->cam_rs_value[c] != 0.) rs_on = true;

    // ---- validate indices ----
    for (int a = 0; a < nA; ++a) require(pr->attr_offset[a] >= 0, "attr_offset");
    for (int t = 0; t < nT; ++t) {
        require(pr->tfm_parent[t] < t, "transforms must be topologically sorted");
        for (int k = 0; k < 9; ++k) require(pr->tfm_attrs[9 * t + k] < nA, "tfm attr id");
    }
    for (int c = 0; c < nC; ++c) {
        require(pr->cam_tfm[c] >= 0 && pr->cam_tfm[c] < nT, "cam_tfm");
        for (int k = 0; k < MMBA_CAM_NUM_ATTRS; ++k)
            require(pr->cam_attrs[MMBA_CAM_NUM_ATTRS * c + k] < nA, "cam attr id");
        if (pr->cam_lens) require(pr->cam_lens[c] < nL, "cam_lens");
    }
    for (int b = 0; b < nB; ++b) require(pr->bnd_tfm[b] >= 0 && pr->bnd_tfm[b] < nT, "bnd_tfm");
    for (int k = 0; k < nK; ++k) {
        require(pr->mkr_cam[k] >= 0 && pr->mkr_cam[k] < nC, "mkr_cam");
        require(pr->mkr_bnd[k] >= 0 && pr->mkr_bnd[k] < nB, "mkr_bnd");
    }
    for (int i = 0; i < M; ++i) {
        require(pr->obs_marker[i] >= 0 && pr->obs_marker[i] < nK, "obs_marker");
        require(pr->obs_frame[i] >= 0 && pr->obs_frame[i] < F, "obs_frame");
        require(pr->obs_weight[i] > 0.0, "obs_weight must be > 0");
    }
    // B4 (mmba.h ABI 8): in MMSG mode observation (marker i, frame f) reads the
    // flat lists at i * F + f, which hold the i-th marker in camera order
    // (flat.rs:271-356, adjust_measureErrors.cpp:454-459).  obs_geo = the
    // marker whose camera, bundle and x,y the observation compares; its weight
    // and lens instance (B3, from obs_marker) are its own.
    std::vector<int> obs_geo(pr->obs_marker, pr->obs_marker + M);
    std::vector<double> obs_xy_geo;  // empty: obs_xy
    // where each observation's x,y comes from (mmba_plan_set_marker_values
    // refreshes it from there): >= 0 an index into obs_xy, < 0 the index
    // -(src + 1) into mkr_frame_xy; empty: its own obs_xy entry
    std::vector<int> obs_xy_src;
    mk_frame_src = false;
    if (opt.scene_graph_mode == MMBA_SCENE_GRAPH_MM_SCENE_GRAPH) {
        std::vector<int> flat;
        flat.reserve(nK);
        for (int c = 0; c < nC; ++c)
            for (int k = 0; k < nK; ++k)
                if (pr->mkr_cam[k] == c) flat.push_back(k);
        bool moved = false;
        for (int k = 0; k < nK; ++k) moved |= flat[k] != k;
        if (moved) {
            if (rs_on) throw Unsupported{"rolling shutter with MMSG markers not grouped by camera (B4)"};
            std::map<std::pair<int, int>, int> obs_at;
            if (!pr->mkr_frame_xy)
                for (int i = 0; i < M; ++i) obs_at[{pr->obs_marker[i], pr->obs_frame[i]}] = i;
            obs_xy_geo.assign(pr->obs_xy, pr->obs_xy + 2 * (size_t)M);
            obs_xy_src.resize(M);
            std::iota(obs_xy_src.begin(), obs_xy_src.end(), 0);
            mk_frame_src = pr->mkr_frame_xy != nullptr;
            if (mk_frame_src) require((long long)nK * F <= INT_MAX, "markers x frames above 2^31");
            for (int i = 0; i < M; ++i) {
                const int k = flat[pr->obs_marker[i]], f = pr->obs_frame[i];
                obs_geo[i] = k;
                if (k == pr->obs_marker[i]) continue;
                const double *xy;
                if (pr->mkr_frame_xy) {
                    xy = &pr->mkr_frame_xy[2 * ((size_t)k * F + f)];
                    obs_xy_src[i] = -(k * F + f) - 1;
                } else {
                    auto it = obs_at.find({k, f});
                    if (it == obs_at.end())
                        throw Unsupported{"MMSG markers not grouped by camera (B4): a flat marker "
                                          "without an observation at the frame read, and no "
                                          "mkr_frame_xy"};
                    xy = &pr->obs_xy[2 * (size_t)it->second];
                    obs_xy_src[i] = it->second;
                }
                obs_xy_geo[2 * i] = xy[0];
                obs_xy_geo[2 * i + 1] = xy[1];
            }
        }
    }
    for (int p = 0; p < n; ++p) {
        const int a = pr->param_attr[p];
        require(a >= 0 && a < nA, "param_attr");
        require(pr->attr_animated[a] ? (pr->param_frame[p] >= 0 && pr->param_frame[p] < F)
                                     : pr->param_frame[p] < 0,
                "param_frame must be -1 for static and a frame for animated attrs");
    }
    param_weight.assign(n, 1.0);
    if (pr->param_weight)
        for (int p = 0; p < n; ++p) param_weight[p] = pr->param_weight[p];
    // stiffness / smoothness rows: the parameter setting each row's
    // (attribute, frame), if any (a static attribute has one parameter)
    std::vector<int> row_attr, row_frame, row_param;
    std::vector<double> row_w, row_var, row_val;
    {
        std::map<std::pair<int, int>, int> attr_param;
        for (int p = 0; p < n; ++p) attr_param[{pr->param_attr[p], pr->param_frame[p]}] = p;
        auto add_rows = [&](int cnt, const int32_t *ra, const int32_t *rf, const double *w,
                            const double *var, const double *val) {
            for (int r = 0; r < cnt; ++r) {
                const int a = ra[r];
                require(a >= 0 && a < nA, "stiffness / smoothness attribute id");
                const int f = pr->attr_animated[a] ? (rf ? rf[r] : 0) : 0;
                require(f >= 0 && f < F, "stiffness / smoothness frame");
                row_attr.push_back(a);
                row_frame.push_back(f);
                row_w.push_back(w[r]);
                row_var.push_back(var[r]);
                row_val.push_back(val[r]);
                auto it = attr_param.find({a, pr->attr_animated[a] ? f : -1});
                row_param.push_back(it == attr_param.end() ? -1 : it->second);
            }
        };
        if (pr->num_stiff > 0)
            add_rows(pr->num_stiff, pr->stiff_attr, pr->stiff_frame, pr->stiff_weight,
                     pr->stiff_variance, pr->stiff_value);
        if (pr->num_smooth > 0)
            add_rows(pr->num_smooth, pr->smooth_attr, pr->smooth_frame, pr->smooth_weight,
                     pr->smooth_variance, pr->smooth_value);
    }
    // the cameras' lenses: one shared lens (or none) is the plain case; with
    // several, the reference's index arithmetic (B3, below) decides which
    // lens instance distorts which observation
    int lens_owner = -2;
    bool several_lenses = false;
    for (int c = 0; c < nC; ++c) {
        const int l = pr->cam_lens ? pr->cam_lens[c] : -1;
        if (l >= 0 && (pr->lens_type[l] < MMBA_LENS_3DE_CLASSIC ||
                       pr->lens_type[l] > MMBA_LENS_3DE_ANAMORPHIC_STD_DEG4_RESCALED))
            throw Unsupported{"unknown lens model type"};
        if (l < 0) continue;
        if (lens_owner == -2) lens_owner = l;
        else if (l != lens_owner) several_lenses = true;
    }
    if (lens_owner == -2) lens_owner = -1;
    if (several_lenses && pr->lens_input)
        for (int c = 0; c < nC; ++c) {
            const int l = pr->cam_lens[c];
            if (l >= 0 && pr->lens_input[l] >= 0)
                throw Unsupported{"input lens layers with several camera lenses"};
        }
    build_lens_instances(pr);
    // ABI 5: the lens's input layers, constants of the solve (mmba.h), deepest
    // first: type, then the 14 slot values (lens_input_values, or each slot's
    // attribute at frame 0; absent slots the model's default)
    std::vector<double> lens_chain_h;
    if (lens_owner >= 0 && pr->lens_input) {
        std::vector<int> lay;
        for (int l = pr->lens_input[lens_owner]; l >= 0; l = pr->lens_input[l]) {
            require(l < nL, "lens_input");
            if (l == lens_owner || std::find(lay.begin(), lay.end(), l) != lay.end())
                throw Unsupported{"cyclic lens input chain"};
            if ((int)lay.size() >= LENS_CHAIN_MAX)
                throw Unsupported{"more than 4 input lens layers"};
            lay.push_back(l);
        }
        for (auto it = lay.rbegin(); it != lay.rend(); ++it) {
            const int l = *it, type = pr->lens_type[l];
            if (type < MMBA_LENS_3DE_CLASSIC || type > MMBA_LENS_3DE_ANAMORPHIC_STD_DEG4_RESCALED)
                throw Unsupported{"unknown lens model type"};
            const bool classic = type == MMBA_LENS_3DE_CLASSIC;
            const bool anam = type == MMBA_LENS_3DE_ANAMORPHIC_STD_DEG4 ||
                              type == MMBA_LENS_3DE_ANAMORPHIC_STD_DEG4_RESCALED;
            lens_chain_h.push_back((double)type);
            for (int k = 0; k < MMBA_LENS_NUM_ATTRS; ++k) {
                double v = ((classic && k == 1) || (anam && k >= 11)) ? 1. : 0.;
                if (pr->lens_input_values) {
                    v = pr->lens_input_values[(size_t)MMBA_LENS_NUM_ATTRS * l + k];
                } else {
                    const int a = pr->lens_attrs[MMBA_LENS_NUM_ATTRS * l + k];
                    if (a >= 0) {
                        require(a < nA, "lens_attrs");
                        v = pr->attr_values[pr->attr_offset[a]];
                    }
                }
                if (type == MMBA_LENS_3DE_ANAMORPHIC_STD_DEG4 && k == 13) v = 1.;  // no rescale slot
                lens_chain_h.push_back(v);
            }
        }
    }

    // ---- attribute -> dependent cameras / bundles / lens-cameras ----
    std::vector<std::vector<int>> chain(nT);
    for (int t = 0; t < nT; ++t) {
        for (int u = t; u >= 0; u = pr->tfm_parent[u]) chain[t].push_back(u);
        if ((int)chain[t].size() > 16) throw Unsupported{"transform hierarchy deeper than 16"};
    }
    std::vector<std::vector<int>> attr_cams(nA), attr_bnds(nA), attr_lcams(nA);
    for (int c = 0; c < nC; ++c) {
        std::set<int> dep;
        for (int t : chain[pr->cam_tfm[c]])
            for (int k = 0; k < 9; ++k) dep.insert(pr->tfm_attrs[9 * t + k]);
        for (int k = 0; k < MMBA_CAM_NUM_ATTRS; ++k) dep.insert(pr->cam_attrs[MMBA_CAM_NUM_ATTRS * c + k]);
        for (int a : dep)
            if (a >= 0) attr_cams[a].push_back(c);
        const int l = pr->cam_lens ? pr->cam_lens[c] : -1;
        if (l >= 0)
            for (int k = 0; k < MMBA_LENS_NUM_ATTRS; ++k) {
                const int a = pr->lens_attrs[MMBA_LENS_NUM_ATTRS * l + k];
                if (a >= 0) attr_lcams[a].push_back(c);
            }
    }
    for (int b = 0; b < nB; ++b) {
        std::set<int> dep;
        const int t0 = pr->bnd_tfm[b];
        for (int k = 0; k < 3; ++k) dep.insert(pr->tfm_attrs[9 * t0 + k]);
        for (size_t q = 1; q < chain[t0].size(); ++q)
            for (int k = 0; k < 9; ++k) dep.insert(pr->tfm_attrs[9 * chain[t0][q] + k]);
        for (int a : dep)
            if (a >= 0) attr_bnds[a].push_back(b);
    }

    // ---- camera-frame keys: every (camera, frame) with observations, keyed
    // (frame, camera) so camera-frames are numbered frame-major: a bundle tracked
    // over a window of frames then couples a contiguous band of the reduced
    // system, for any number of cameras ----
    std::vector<int> obs_cam(M);
    for (int i = 0; i < M; ++i) obs_cam[i] = pr->mkr_cam[obs_geo[i]];
    std::map<std::pair<int, int>, int> cf_id;
    for (int i = 0; i < M; ++i) cf_id[{pr->obs_frame[i], obs_cam[i]}] = 0;

    // ---- an animated lens coefficient whose Jacobian column reaches the
    // rows of ONE camera-frame (the column re-measures its own frame only,
    // adjust_solveFunc.cpp frameIndexEnable; its lens instances at that
    // frame are read by one camera: one camera per lens, or B3's index
    // arithmetic keeping the writes on it) joins that camera-frame's block
    // instead of the global arrow (VERDICT r4 "next" 7: focus breathing over
    // more than NGMAX frames).  Forward differences, no rolling shutter ----
    std::vector<int> lens_cam(n, -2);  // -2: no reader, -1: several cameras
    std::vector<std::set<int>> lens_readers(n);  // the cameras whose rows read it at its frame
    if (!rs_on && !central && path_choice(MMBA_PATH_LENS_CF) != 0 && !inst_lens_h.empty()) {
        require(M == Mg, "lens classification before sharding");
        for (int r = 0; r < Mg; ++r) {
            const int j = obs_inst_g[r];
            if (j < 0) continue;
            for (int q = inst_lpar_off_h[j]; q < inst_lpar_off_h[j + 1]; ++q) {
                const int p = inst_lpar_h[q];
                if (pr->param_frame[p] != pr->obs_frame[r]) continue;
                int &c = lens_cam[p];
                c = c == -2 ? obs_cam[r] : (c == obs_cam[r] ? c : -1);
                lens_readers[p].insert(obs_cam[r]);
            }
        }
    }
    // ---- ... and one whose column reaches the rows of SEVERAL cameras at
    // its frame (two cameras on one lens, C5 with focus breathing): the shared
    // form puts it into the block of the frame's lowest-numbered reading
    // camera-frame, its host; the other readers are foreign -- their rows
    // carry its column beside their own block's (k_jacobian's lens loop) and
    // couple their camera-frame to the host's through an off-diagonal block
    // (mmba_lens_shared.hip).  A coefficient no row reads at its frame (a zero
    // column) is then hosted by the frame's first camera-frame.  Taken where
    // the global form would exceed NGMAX (MMBA_PATH_LENS_SHARED = 1: wherever
    // eligible, 0: never); needs what the one-camera form needs, one device
    // and no solved bundle (a foreign row's W row would span two blocks) ----
    bool has_anim_lens = false, has_solved_bundle = false;
    for (int p = 0; p < n; ++p) {
        const int a = pr->param_attr[p];
        if (!attr_lcams[a].empty() && pr->param_frame[p] >= 0) has_anim_lens = true;
        if (attr_lcams[a].empty() && attr_cams[a].empty() && attr_bnds[a].size() == 1 &&
            pr->param_frame[p] < 0)
            has_solved_bundle = true;
    }
    const int shared_pin = path_choice(MMBA_PATH_LENS_SHARED);
    const char *shared_off = nullptr;  // the condition that keeps the shared form off
    if (path_choice(MMBA_PATH_LENS_CF) == 0) shared_off = "MMBA_PATH_LENS_CF = 0";
    else if (shared_pin == 0) shared_off = "MMBA_PATH_LENS_SHARED = 0";
    else if (rs_on) shared_off = "rolling shutter";
    else if (central) shared_off = "central differences";
    else if (nranks > 1) shared_off = "sharded plan";
    else if (has_solved_bundle) shared_off = "solved bundles";
    // the host camera of a shared coefficient, -1: it stays global
    auto shared_host = [&](int p) -> int {
        if (lens_cam[p] == -1) return *lens_readers[p].begin();
        auto it = cf_id.lower_bound({pr->param_frame[p], INT32_MIN});  // lens_cam -2: no reader
        return (it != cf_id.end() && it->first.first == pr->param_frame[p]) ? it->first.second : -1;
    };
    // ---- an object-frame parameter: an animated transform attribute above
    // bundles and above no camera (a rigid object keyed per frame, its
    // bundles parented under it).  Its column re-measures its own frame only
    // (frameIndexEnable, as above), so it reaches the rows of that frame whose
    // bundle hangs under the transform.  Read there by ONE camera it joins
    // that camera-frame's block (VF_OBJ) instead of the global arrow; read by
    // no row (the object unseen at the frame: a zero column) it is hosted by
    // the frame's first camera-frame, as the shared lens form hosts its
    // unread coefficients; read by several cameras it stays global.  Taken
    // where the global form would exceed NGMAX (MMBA_PATH_OBJ_CF = 1: wherever
    // eligible, 0: never).  Forward differences, no rolling shutter, no
    // robust loss, one device ----
    std::vector<int> obj_cam(n, -3);  // -3: no such parameter, -2: no reader, -1: several cameras
    bool has_obj = false, obj_several = false;
    for (int p = 0; p < n; ++p) {
        const int a = pr->param_attr[p];
        if (pr->param_frame[p] >= 0 && attr_lcams[a].empty() && attr_cams[a].empty() &&
            !attr_bnds[a].empty()) {
            obj_cam[p] = -2;
            has_obj = true;
        }
    }
    const int obj_pin = path_choice(MMBA_PATH_OBJ_CF);
    const char *obj_off = nullptr;  // the condition that keeps them global
    if (obj_pin == 0) obj_off = "MMBA_PATH_OBJ_CF = 0";
    else if (rs_on) obj_off = "rolling shutter";
    else if (central) obj_off = "central differences";
    else if (opt.robust_loss) obj_off = "robust loss";
    else if (nranks > 1) obj_off = "sharded plan";
    if (has_obj && !obj_off) {
        require(M == Mg, "object classification before sharding");
        std::vector<std::vector<int>> frame_obs(F);
        for (int r = 0; r < Mg; ++r) frame_obs[pr->obs_frame[r]].push_back(r);
        std::map<int, std::vector<char>> under;  // attribute -> its bundles, as a mask
        for (int p = 0; p < n; ++p) {
            if (obj_cam[p] == -3) continue;
            const int a = pr->param_attr[p];
            auto it = under.find(a);
            if (it == under.end()) {
                it = under.emplace(a, std::vector<char>(nB, 0)).first;
                for (int b : attr_bnds[a]) it->second[b] = 1;
            }
            for (int r : frame_obs[pr->param_frame[p]]) {
                if (!it->second[pr->mkr_bnd[obs_geo[r]]]) continue;
                int &c = obj_cam[p];
                c = c == -2 ? obs_cam[r] : (c == obs_cam[r] ? c : -1);
            }
            if (obj_cam[p] == -1) obj_several = true;
        }
    }
    // the camera whose camera-frame hosts an object-frame parameter, -1: global
    auto obj_host = [&](int p) -> int {
        if (obj_cam[p] >= 0) return obj_cam[p];
        if (obj_cam[p] != -2) return -1;
        auto it = cf_id.lower_bound({pr->param_frame[p], INT32_MIN});
        return (it != cf_id.end() && it->first.first == pr->param_frame[p]) ? it->first.second : -1;
    };
    // ---- classify parameters ----
    std::vector<int> p_class(n), p_blk(n, -1), p_pos(n, -1), p_both(n, 0), p_lens(n, 0);
    std::vector<int> p_shared(n, 0);  // hosted in the shared form
    std::vector<int> p_obj(n, 0);     // an object-frame parameter in a camera-frame block
    std::vector<std::pair<int, int>> p_cfkey(n, {-1, -1});
    lens_shared = false;
    bool obj_form = false;  // object-frame parameters join the blocks
    // shared: the several-camera form too; returns the number of globals
    auto classify = [&](bool shared) -> int {
        int ng = 0;
        for (int p = 0; p < n; ++p) {
            const int a = pr->param_attr[p], fp = pr->param_frame[p];
            const auto &cams = attr_cams[a];
            const auto &bnds = attr_bnds[a];
            const auto &lc = attr_lcams[a];
            if (!lc.empty() && (!cams.empty() || !bnds.empty()))
                throw Unsupported{"attribute used both as lens coefficient and geometry"};
            p_both[p] = (!cams.empty() && !bnds.empty()) ? 1 : 0;
            if (lc.empty() && bnds.empty() && cams.size() == 1 && fp >= 0) {
                p_class[p] = PC_CF;
                p_cfkey[p] = {fp, cams[0]};
                cf_id[{fp, cams[0]}] = 0;
            } else if (lc.empty() && cams.empty() && bnds.size() == 1 && fp < 0) {
                p_class[p] = PC_B;
                p_blk[p] = bnds[0];
            } else if (!lc.empty() && fp >= 0 && lens_cam[p] >= 0) {
                p_class[p] = PC_CF;
                p_lens[p] = 1;
                p_cfkey[p] = {fp, lens_cam[p]};
            } else if (shared && !lc.empty() && fp >= 0 && shared_host(p) >= 0) {
                p_class[p] = PC_CF;
                p_lens[p] = 1;
                p_shared[p] = 1;
                p_cfkey[p] = {fp, shared_host(p)};
                if (lens_cam[p] == -1) lens_shared = true;
            } else if (obj_form && obj_host(p) >= 0) {
                p_class[p] = PC_CF;
                p_obj[p] = 1;
                p_cfkey[p] = {fp, obj_host(p)};
            } else {
                p_class[p] = PC_G;
                ++ng;
            }
        }
        return ng;
    };
    // the forms taken so far first; the object form and the shared form
    // where they leave more than NGMAX globals, or where they are pinned on
    int ng_plain = classify(false);
    if (has_obj && !obj_off && (obj_pin == 1 || t_obj_cf || ng_plain > NGMAX)) {
        obj_form = true;
        ng_plain = classify(false);
    }
    if (!shared_off && has_anim_lens && !inst_lens_h.empty() &&
        (shared_pin == 1 || ng_plain > NGMAX))
        classify(true);
    if (!lens_shared)  // no coefficient with several readers: nothing changes
        for (int p = 0; p < n; ++p)
            if (p_shared[p]) {
                p_class[p] = PC_G;
                p_lens[p] = p_shared[p] = 0;
                p_cfkey[p] = {-1, -1};
            }
    // number the camera-frames: frame-major (the keys' order), so a bundle
    // tracked over a window of frames couples a contiguous band; with a
    // rolling shutter and no solved bundle, camera-major instead: the
    // coupling is then only between a camera's consecutive frames, and the
    // band is 3 camera-frame blocks wide whatever the number of cameras
    // (C5-RS: half bandwidth 17 instead of 29)
    ncf = 0;
    std::vector<int> cf_cam, cf_frame;
    {
        bool any_b = false;
        for (int p = 0; p < n && !any_b; ++p) any_b = p_class[p] == PC_B;
        std::vector<std::pair<int, int>> keys;
        for (auto &kv : cf_id) keys.push_back(kv.first);
        if (rs_on && !any_b)
            std::stable_sort(keys.begin(), keys.end(),
                             [](const std::pair<int, int> &a, const std::pair<int, int> &b) {
                                 return a.second != b.second ? a.second < b.second
                                                             : a.first < b.first;
                             });
        for (auto &k : keys) {
            cf_id[k] = ncf++;
            cf_frame.push_back(k.first);
            cf_cam.push_back(k.second);
        }
    }
    // CF blocks
    std::vector<std::vector<int>> cf_params(ncf);
    for (int p = 0; p < n; ++p)
        if (p_class[p] == PC_CF) {
            const int cf = cf_id[p_cfkey[p]];
            p_blk[p] = cf;
            cf_params[cf].push_back(p);
        }
    std::vector<int> cf_pc(ncf), cf_roff(ncf);
    nCF = 0;
    for (int cf = 0; cf < ncf; ++cf) {
        cf_pc[cf] = (int)cf_params[cf].size();
        if (cf_pc[cf] > PCMAX)
            throw Unsupported{"more than " + std::to_string(PCMAX) +
                              " parameters on one camera-frame"};
        cf_roff[cf] = nCF;
        for (int a = 0; a < cf_pc[cf]; ++a) p_pos[cf_params[cf][a]] = nCF + a;
        nCF += cf_pc[cf];
    }
    // globals
    std::vector<int> g_param;
    for (int p = 0; p < n; ++p)
        if (p_class[p] == PC_G) g_param.push_back(p);
    nG = (int)g_param.size();
    if (nG > NGMAX)
        throw Unsupported{"more than " + std::to_string(NGMAX) + " global parameters" +
                          (has_anim_lens && shared_off
                               ? std::string(" (animated lens coefficients shared by several "
                                             "cameras stay global parameters: ") +
                                     shared_off + ")"
                               : std::string()) +
                          (has_obj && obj_off
                               ? std::string(" (animated transforms above bundles stay global "
                                             "parameters: ") +
                                     obj_off + ")"
                               : std::string()) +
                          (obj_form && obj_several
                               ? std::string(" (an animated transform above bundles seen by "
                                             "several cameras at one frame stays a global "
                                             "parameter per frame)")
                               : std::string())};
    for (int q = 0; q < nG; ++q) p_pos[g_param[q]] = nCF + q;
    nR = nCF + nG;

    // camera variants: base, CF-block params, cam-side globals valid at the frame
    std::vector<int> cf_var_off(ncf + 1, 0), cf_var_param, cf_var_flags, var_cf;
    for (int cf = 0; cf < ncf; ++cf) {
        cf_var_off[cf] = (int)cf_var_param.size();
        cf_var_param.push_back(-1);
        cf_var_flags.push_back(0);
        var_cf.push_back(cf);
        for (int p : cf_params[cf]) {
            cf_var_param.push_back(p);
            cf_var_flags.push_back(p_lens[p]  ? VF_LENS
                                   : p_obj[p] ? (VF_OBJ | VF_BUNDLE_SIDE)
                                              : (p_both[p] ? VF_BUNDLE_SIDE : 0));
            var_cf.push_back(cf);
        }
        for (int p : g_param) {
            const int a = pr->param_attr[p], fp = pr->param_frame[p];
            if (fp >= 0 && fp != cf_frame[cf]) continue;
            const auto &cams = attr_cams[a];
            if (std::find(cams.begin(), cams.end(), cf_cam[cf]) == cams.end()) continue;
            cf_var_param.push_back(p);
            cf_var_flags.push_back(p_both[p] ? VF_BUNDLE_SIDE : 0);
            var_cf.push_back(cf);
        }
    }
    cf_var_off[ncf] = (int)cf_var_param.size();
    nvar = cf_var_off[ncf];

    // bundle-side lists: B params first, then bundle-side globals
    std::vector<std::vector<int>> bpar(nB);
    for (int p = 0; p < n; ++p)
        if (p_class[p] == PC_B) bpar[p_blk[p]].push_back(p);
    std::vector<int> bnd_pb(nB), bnd_par_off(nB + 1, 0), bnd_par;
    nB_solved = 0;
    for (int b = 0; b < nB; ++b) {
        bnd_pb[b] = (int)bpar[b].size();
        if (bnd_pb[b] > PBMAX) throw Unsupported{"more than 3 parameters on one bundle"};
        if (bnd_pb[b] > 0) ++nB_solved;
        for (int a = 0; a < bnd_pb[b]; ++a) p_pos[bpar[b][a]] = a;
    }
    std::vector<std::vector<int>> bglob(nB);
    for (int p : g_param)
        for (int b : attr_bnds[pr->param_attr[p]]) bglob[b].push_back(p);
    for (int b = 0; b < nB; ++b) {
        bnd_par_off[b] = (int)bnd_par.size();
        for (int p : bpar[b]) bnd_par.push_back(p);
        for (int p : bglob[b]) bnd_par.push_back(p);
    }
    bnd_par_off[nB] = (int)bnd_par.size();
    // fast bundles: position independent of the frame (no animated attribute
    // in the bundle's transform chain) and only B-class parameters
    std::vector<int4> bnd_p4(nB);
    for (int b = 0; b < nB; ++b) {
        bool fast = bglob[b].empty();
        const int t0 = pr->bnd_tfm[b];
        for (size_t q = 0; q < chain[t0].size() && fast; ++q)
            for (int k = 0; k < (q == 0 ? 3 : 9); ++k) {
                const int a = pr->tfm_attrs[9 * chain[t0][q] + k];
                if (a >= 0 && pr->attr_animated[a]) fast = false;
            }
        const auto &bp = bpar[b];
        bnd_p4[b] = make_int4(bp.size() > 0 ? bp[0] : -1, bp.size() > 1 ? bp[1] : -1,
                              bp.size() > 2 ? bp[2] : -1, fast ? (int)bp.size() : -1);
    }
    // lens params per camera
    std::vector<int> cam_lpar_off(nC + 1, 0), cam_lpar;
    for (int c = 0; c < nC; ++c) {
        cam_lpar_off[c] = (int)cam_lpar.size();
        for (int p : g_param) {
            const auto &lc = attr_lcams[pr->param_attr[p]];
            if (std::find(lc.begin(), lc.end(), c) != lc.end()) cam_lpar.push_back(p);
        }
    }
    cam_lpar_off[nC] = (int)cam_lpar.size();

    // ---- reduced-system layout: band + arrow when the camera-frame band is
    // narrow (every C2/C4/C5-like scene), 64x64 tiles otherwise.  Computed from
    // all observations so every shard sees the same structure. ----
    std::vector<int> obs_cf(Mg);
    for (int i = 0; i < Mg; ++i) obs_cf[i] = cf_id[{pr->obs_frame[i], obs_cam[i]}];
    std::vector<int> obs_bnd_g(Mg);
    for (int i = 0; i < Mg; ++i) obs_bnd_g[i] = pr->mkr_bnd[obs_geo[i]];
    // rolling shutter: the camera-frames of the same camera at f - 1 / f + 1
    // (cameras with rs != 0), whose translate / rotate values the blend reads
    std::vector<int> cf_nb(2 * (size_t)std::max(ncf, 1), -1);
    if (rs_on) {
        if (nranks > 1) throw Unsupported{"rolling shutter: sharded solve"};
        if (central) throw Unsupported{"rolling shutter with central differences"};
        for (int b = 0; b < nB; ++b)
            if (!bglob[b].empty()) throw Unsupported{"rolling shutter with bundle-side global parameters"};
        for (int v : cf_var_flags)
            if (v != 0) throw Unsupported{"rolling shutter with a camera / bundle shared attribute"};
        for (int cf = 0; cf < ncf; ++cf) {
            const int c = cf_cam[cf], f = cf_frame[cf];
            if (pr->cam_rs_value[c] == 0.) continue;
            auto a = cf_id.find({f - 1, c}), b = cf_id.find({f + 1, c});
            if (a != cf_id.end()) cf_nb[2 * cf] = a->second;
            if (b != cf_id.end()) cf_nb[2 * cf + 1] = b->second;
        }
    }
    bw = 0;
    for (int cf = 0; cf < ncf; ++cf)
        if (cf_pc[cf] > 0) bw = std::max(bw, cf_pc[cf] - 1);
    // shared lens coefficients: per host camera-frame the coefficients its
    // block hosts and the foreign camera-frames whose rows read one of them
    // (links); a link couples the foreign block with the hosted rows
    std::vector<int> ls_host, ls_nh, ls_link_off(1, 0), ls_hpar, ls_hpos, ls_link_cf, ls_link_grp;
    if (lens_shared)
        for (int cf = 0; cf < ncf; ++cf) {
            std::vector<int> hosted;
            std::set<int> foreign;
            for (int p : cf_params[cf]) {
                if (!p_shared[p]) continue;
                hosted.push_back(p);
                for (int c : lens_readers[p])
                    if (c != cf_cam[cf]) foreign.insert(cf_id[{cf_frame[cf], c}]);
            }
            if (hosted.empty() || foreign.empty()) continue;
            const int grp = (int)ls_host.size();
            ls_host.push_back(cf);
            ls_nh.push_back((int)hosted.size());
            int lo = nCF;
            for (int h = 0; h < PCMAX; ++h) {
                ls_hpar.push_back(h < (int)hosted.size() ? hosted[h] : -1);
                ls_hpos.push_back(h < (int)hosted.size() ? p_pos[hosted[h]] - cf_roff[cf] : 0);
                if (h < (int)hosted.size()) lo = std::min(lo, p_pos[hosted[h]]);
            }
            for (int x : foreign) {
                // the coupling block sits below the diagonal (k_lens_shared_offdiag)
                if (x <= cf) throw Invalid{"shared lens coefficient: host after a reader"};
                ls_link_cf.push_back(x);
                ls_link_grp.push_back(grp);
                if (cf_pc[x] > 0) bw = std::max(bw, cf_roff[x] + cf_pc[x] - 1 - lo);
            }
            ls_link_off.push_back((int)ls_link_cf.size());
        }
    if (rs_on)  // an observation couples its camera-frame with both neighbours
        for (int cf = 0; cf < ncf; ++cf) {
            int lo = cf_pc[cf] > 0 ? cf_roff[cf] : nCF, hi = cf_pc[cf] > 0 ? cf_roff[cf] + cf_pc[cf] - 1 : -1;
            for (int side = 0; side < 2; ++side) {
                const int cn = cf_nb[2 * cf + side];
                if (cn < 0 || cf_pc[cn] == 0) continue;
                lo = std::min(lo, cf_roff[cn]);
                hi = std::max(hi, cf_roff[cn] + cf_pc[cn] - 1);
            }
            if (hi >= lo) bw = std::max(bw, hi - lo);
        }
    {
        std::vector<int> blo(nB, nCF), bhi(nB, -1);
        for (int i = 0; i < Mg; ++i) {
            const int b = obs_bnd_g[i];
            if (bnd_pb[b] == 0) continue;
            // a rolling-shutter row also reaches the neighbouring frames' blocks
            const int cfs[3] = {obs_cf[i], rs_on ? cf_nb[2 * obs_cf[i]] : -1,
                                rs_on ? cf_nb[2 * obs_cf[i] + 1] : -1};
            for (int cf : cfs) {
                if (cf < 0 || cf_pc[cf] == 0) continue;
                blo[b] = std::min(blo[b], cf_roff[cf]);
                bhi[b] = std::max(bhi[b], cf_roff[cf] + cf_pc[cf] - 1);
            }
        }
        for (int b = 0; b < nB; ++b)
            if (bhi[b] >= 0) bw = std::max(bw, bhi[b] - blo[b]);
    }
    band = nR > 0 && bw <= WBAND_MAX;
    if (rs_on && !band) throw Unsupported{"rolling shutter: camera-frame band wider than WBAND_MAX (80)"};
    if (lens_shared && !band)
        throw Unsupported{"animated lens coefficients shared by several cameras: camera-frame "
                          "band wider than WBAND_MAX (80)"};

    // ---- frame sharding: this shard's frames, camera-frame rows, observations
    // (own = in its frames; halo = other observations of solved bundles seen in
    // its frames, so those bundles' blocks are complete here) ----
    std::vector<int> obs_own_g(Mg, 1), bnd_owner(nB, 0);
    Ra = 0;
    Rb = nCF;
    Ra_all.assign(1, 0);
    Rb_all.assign(1, nCF);
    std::vector<int> local;  // global observation indices on this shard
    std::vector<int> cf_own(ncf, 1);
    // sharded: every global observation's and camera-frame's owning shard
    // (the hand-back lists, setup_handback)
    std::vector<int> obs_rank_g, cf_rank;
    if (nranks > 1) {
        // a camera-frame band wider than the partitioned solvers take (C3:
        // bundles tracked across the whole shot): each shard still assembles
        // the reduced rows of its own camera-frames, the shards' dense S are
        // all-reduced and every shard factors it with the dense solver
        // (Plan::shard_dense)
        shard_dense = !band || bw > WBAND_PART;
        if (shard_dense) {
            band = false;
            if (nR > 65536) throw Unsupported{"sharded dense reduced system above 65,536 rows"};
        }
        std::vector<int> bf(nranks + 1, F), bnd_owner_all(nB, 0);
        shard_layout(F, Mg, pr->obs_frame, obs_bnd_g.data(), nB, nranks, bf.data(),
                     bnd_owner_all.data());
        // camera-frame rows of every shard's frame range (rows are frame-major)
        std::vector<int> first_row(F + 1, nCF);
        for (int cf = ncf - 1; cf >= 0; --cf) first_row[cf_frame[cf]] = cf_roff[cf];
        for (int f = F - 1; f >= 0; --f) first_row[f] = std::min(first_row[f], first_row[f + 1]);
        Ra_all.assign(nranks, 0);
        Rb_all.assign(nranks, 0);
        for (int k = 0; k < nranks; ++k) {
            Ra_all[k] = first_row[bf[k]];
            Rb_all[k] = first_row[bf[k + 1]];
            if (Rb_all[k] - Ra_all[k] < (shard_dense ? 1 : 2 * bw + 8))
                throw Unsupported{"too few camera-frame rows per shard"};
        }
        Ra = Ra_all[rank];
        Rb = Rb_all[rank];
        const int fa = bf[rank], fb = bf[rank + 1];
        for (int cf = 0; cf < ncf; ++cf) cf_own[cf] = (cf_frame[cf] >= fa && cf_frame[cf] < fb);
        for (int i = 0; i < Mg; ++i) {
            const int f = pr->obs_frame[i];
            obs_own_g[i] = (f >= fa && f < fb) ? 1 : 0;
        }
        std::vector<int> frame_rank(F, nranks - 1);
        for (int k = 0; k < nranks; ++k)
            for (int f = bf[k]; f < bf[k + 1]; ++f) frame_rank[f] = k;
        obs_rank_g.resize((size_t)Mg + n);
        for (int i = 0; i < Mg; ++i) obs_rank_g[i] = frame_rank[pr->obs_frame[i]];
        cf_rank.resize(ncf);
        for (int cf = 0; cf < ncf; ++cf) cf_rank[cf] = frame_rank[cf_frame[cf]];
        bnd_owner = bnd_owner_all;
        std::vector<char> bnd_here(nB, 0);
        for (int i = 0; i < Mg; ++i)
            if (obs_own_g[i] && bnd_pb[obs_bnd_g[i]] > 0) bnd_here[obs_bnd_g[i]] = 1;
        for (int i = 0; i < Mg; ++i)
            if (obs_own_g[i] || bnd_here[obs_bnd_g[i]]) local.push_back(i);
        M = (int)local.size();
        m = 2 * M;
    } else {
        local.resize(Mg);
        std::iota(local.begin(), local.end(), 0);
    }

    // ---- local observations in device order (by camera-frame) ----
    ref_of_dev = local;
    std::stable_sort(ref_of_dev.begin(), ref_of_dev.end(),
                     [&](int a, int b) { return obs_cf[a] < obs_cf[b]; });
    std::vector<int> d_cf(M), d_bnd(M), d_frame(M), d_cam(M), d_own(M), d_inst(M);
    std::vector<double> d_xy(2 * (size_t)M), d_sqrtw(M);
    std::vector<int> cf_obs_off(ncf + 1, 0);
    for (int i = 0; i < M; ++i) {
        const int r = ref_of_dev[i];
        d_cf[i] = obs_cf[r];
        d_bnd[i] = obs_bnd_g[r];
        d_frame[i] = pr->obs_frame[r];
        d_cam[i] = obs_cam[r];
        const double *xy = obs_xy_geo.empty() ? pr->obs_xy : obs_xy_geo.data();
        d_xy[2 * i] = xy[2 * r];
        d_xy[2 * i + 1] = xy[2 * r + 1];
        d_sqrtw[i] = std::sqrt(pr->obs_weight[r]);
        d_own[i] = obs_own_g[r];
        d_inst[i] = obs_inst_g[r];
        cf_obs_off[d_cf[i] + 1]++;
    }
    for (int cf = 0; cf < ncf; ++cf) cf_obs_off[cf + 1] += cf_obs_off[cf];
    // local column bound (rolling shutter: + the neighbouring frames' CF blocks)
    // lens parameters that reach an observation: those its lens instance holds
    auto lens_cols = [&](int i) {
        const int j = d_inst[i];
        return j < 0 ? 0 : inst_lpar_off_h[j + 1] - inst_lpar_off_h[j];
    };
    auto obs_cols = [&](int i) {
        const int cf = d_cf[i];
        int nl = (cf_var_off[cf + 1] - cf_var_off[cf] - 1) + lens_cols(i);
        // the bundle-side parameters valid at the observation's frame (an
        // animated one emits its column in its own frame's rows only)
        for (int t = bnd_par_off[d_bnd[i]]; t < bnd_par_off[d_bnd[i] + 1]; ++t)
            if (pr->param_frame[bnd_par[t]] < 0 || pr->param_frame[bnd_par[t]] == d_frame[i]) ++nl;
        for (int side = 0; side < 2; ++side)
            if (cf_nb[2 * cf + side] >= 0) nl += cf_pc[cf_nb[2 * cf + side]];
        return nl;
    };
    for (int i = 0; i < M; ++i)
        if (obs_cols(i) > LMAX) throw Unsupported{"more than 32 parameters reach one observation"};
    // Central differences and the robust loss where an lmder FD column skips
    // marker rows (another frame than an animated parameter's): the
    // reference zero-initialises errorListB (adjust_solveFunc.cpp:412), so a
    // skipped row j of an animated central column p gets f_j c_p,
    // c_p = 0.5 / (|dA| + |dB|) (errorListA keeps f, :331-333, 468-471) --
    // J = J_s + f c^T, a rank-one term (B15, Plan::b15).  That needs every
    // row of the column's own frame to be one the column reaches (else J_s
    // would gain entries outside the block structure); the robust loss
    // re-applies the loss to the whole buffer (adjust_measureErrors.cpp:
    // 553-558) and stays refused there.
    b15 = false;
    if (lmder_opt && (central || opt.robust_loss)) {
        int fmin = F, fmax = -1;
        for (int i = 0; i < Mg; ++i) {
            fmin = std::min(fmin, (int)pr->obs_frame[i]);
            fmax = std::max(fmax, (int)pr->obs_frame[i]);
        }
        bool masked = false;
        for (int p = 0; p < n && !masked; ++p)
            if (pr->param_frame[p] >= 0 && (fmin != pr->param_frame[p] || fmax != fmin))
                masked = true;
        const bool skips = masked;  // some animated column skips another frame's rows
        for (int i = 0; i < M && !masked; ++i) {
            const int cf = d_cf[i];
            const int nl = (cf_var_off[cf + 1] - cf_var_off[cf] - 1) +
                           (bnd_par_off[d_bnd[i] + 1] - bnd_par_off[d_bnd[i]]) + lens_cols(i);
            if (nl == 0) masked = true;
        }
        if (masked && central && !opt.robust_loss && nranks == 1 && nrows == 0 && !rs_on) {
            // every observation of an animated parameter's frame reached by it
            std::vector<std::vector<int>> anim_at(F);
            for (int p = 0; p < n; ++p)
                if (pr->param_frame[p] >= 0) anim_at[pr->param_frame[p]].push_back(p);
            // ... and every animated parameter a camera-frame block parameter
            // (the rotated basis lives in those blocks)
            bool cover = true;
            for (int p = 0; p < n; ++p)
                if (pr->param_frame[p] >= 0 && p_class[p] != PC_CF) cover = false;
            std::vector<int> reach;
            for (int i = 0; i < M && cover; ++i) {
                const auto &need = anim_at[d_frame[i]];
                if (need.empty()) continue;
                reach.clear();
                const int cf = d_cf[i];
                for (int t = cf_var_off[cf] + 1; t < cf_var_off[cf + 1]; ++t)
                    reach.push_back(cf_var_param[t]);
                for (int t = bnd_par_off[d_bnd[i]]; t < bnd_par_off[d_bnd[i] + 1]; ++t)
                    reach.push_back(bnd_par[t]);
                if (d_inst[i] >= 0)
                    for (int q = inst_lpar_off_h[d_inst[i]]; q < inst_lpar_off_h[d_inst[i] + 1]; ++q)
                        reach.push_back(inst_lpar_h[q]);
                for (int p : need)
                    if (std::find(reach.begin(), reach.end(), p) == reach.end()) cover = false;
            }
            if (cover) {  // (rows no column reaches stay zero rows of J)
                b15 = skips;
                masked = false;
            }
        }
        if (masked)
            throw Unsupported{std::string(central ? "central differences" : "robust loss") +
                              " with lmder where an FD column skips marker rows (animated "
                              "parameters over several frames) and its own frame holds rows it "
                              "does not reach, or with the robust loss, attribute rows, the "
                              "rolling shutter or shards (B15)"};
    }
    // observations grouped by bundle
    std::vector<int> bobs_off(nB + 1, 0), bobs(M);
    for (int i = 0; i < M; ++i) bobs_off[d_bnd[i] + 1]++;
    for (int b = 0; b < nB; ++b) bobs_off[b + 1] += bobs_off[b];
    {
        std::vector<int> fill(bobs_off.begin(), bobs_off.end() - 1);
        for (int i = 0; i < M; ++i) bobs[fill[d_bnd[i]]++] = i;
    }
    // rolling shutter with solved bundles: a row reaches the camera-frame
    // blocks of f - 1, f, f + 1, so the Schur complement runs over virtual
    // observations -- one per (observation, block it reaches) with its own W
    // row (k_schur_obs_rs), grouped by camera-frame and by bundle like the
    // real ones; the Schur kernels take that view (PV) unchanged
    rs_bnd = rs_on && nB_solved > 0;
    std::vector<int> v_obs, v_cf, v_bnd, v_coff, vcf_off(ncf + 1, 0), vbobs, vbobs_off(nB + 1, 0);
    if (rs_bnd) {
        struct VObs {
            int cf, i, coff;
        };
        std::vector<VObs> vs;
        for (int i = 0; i < M; ++i) {
            if (bnd_pb[d_bnd[i]] == 0) continue;
            const int cf = d_cf[i], pp = cf_nb[2 * cf], nn = cf_nb[2 * cf + 1];
            const int nvs = cf_var_off[cf + 1] - cf_var_off[cf] - 1;  // k_jacobian_rs's order
            if (cf_pc[cf] > 0) vs.push_back({cf, i, 0});
            if (pp >= 0 && cf_pc[pp] > 0) vs.push_back({pp, i, nvs});
            if (nn >= 0 && cf_pc[nn] > 0) vs.push_back({nn, i, nvs + (pp >= 0 ? cf_pc[pp] : 0)});
        }
        std::stable_sort(vs.begin(), vs.end(), [](const VObs &a, const VObs &b) { return a.cf < b.cf; });
        Mv = (int)vs.size();
        for (const VObs &v : vs) {
            v_obs.push_back(v.i);
            v_cf.push_back(v.cf);
            v_bnd.push_back(d_bnd[v.i]);
            v_coff.push_back(v.coff);
            vcf_off[v.cf + 1]++;
            vbobs_off[d_bnd[v.i] + 1]++;
        }
        for (int cf = 0; cf < ncf; ++cf) vcf_off[cf + 1] += vcf_off[cf];
        for (int b = 0; b < nB; ++b) vbobs_off[b + 1] += vbobs_off[b];
        vbobs.assign(std::max(Mv, 1), 0);
        std::vector<int> fill(vbobs_off.begin(), vbobs_off.end() - 1);
        for (int v = 0; v < Mv; ++v) vbobs[fill[v_bnd[v]]++] = v;
    }
    // stale errorDistanceList source per frame (B13): last parameter whose
    // frame mask includes the frame; lmdif re-measures everything per column.
    std::vector<int> stale(F, -1);
    for (int f = 0; f < F; ++f) {
        if (opt.solver_type == MMBA_SOLVER_CMINPACK_LMDIF) {
            stale[f] = n - 1;
            continue;
        }
        for (int p = n - 1; p >= 0; --p)
            if (pr->param_frame[p] < 0 || pr->param_frame[p] == f ||
                (rs_on && std::abs(pr->param_frame[p] - f) <= 1)) {
                stale[f] = p;
                break;
            }
    }
    stale_host = stale;
    param_frame_host.assign(pr->param_frame, pr->param_frame + n);
    pmin_h.assign(pr->param_min, pr->param_min + n);
    pmax_h.assign(pr->param_max, pr->param_max + n);
    poff_h.assign(pr->param_offset, pr->param_offset + n);
    pscale_h.assign(pr->param_scale, pr->param_scale + n);
    param_vidx.resize(n);
    for (int p = 0; p < n; ++p) {
        const int a = pr->param_attr[p];
        param_vidx[p] = pr->attr_offset[a] + (pr->attr_animated[a] ? pr->param_frame[p] : 0);
    }

    // ---- symbolic tile structure of the reduced system ----
    NT = (nR > 0 && !band) ? (nR + TILE - 1) / TILE : 0;
    nRpad = band ? nR : NT * TILE;
    std::vector<uint8_t> nz((size_t)NT * NT, 0);
    auto mark = [&](int R, int C) {
        if (NT == 0) return;
        int I = R / TILE, J = C / TILE;
        if (I < J) std::swap(I, J);
        nz[(size_t)I * NT + J] = 1;
    };
    for (int I = 0; I < NT; ++I) nz[(size_t)I * NT + I] = 1;
    for (int cf = 0; cf < ncf; ++cf)
        if (cf_pc[cf] > 0) {
            mark(cf_roff[cf], cf_roff[cf]);
            mark(cf_roff[cf] + cf_pc[cf] - 1, cf_roff[cf]);
            mark(cf_roff[cf] + cf_pc[cf] - 1, cf_roff[cf] + cf_pc[cf] - 1);
        }
    if (nG > 0)
        for (int R = nCF; R < nR; R += 1)
            for (int J = 0; J < NT; ++J) {
                int I = R / TILE;
                if (J <= I) nz[(size_t)I * NT + J] = 1;
            }
    for (int b = 0; b < nB && NT > 0; ++b) {
        if (bnd_pb[b] == 0) continue;
        std::set<int> tiles;
        for (int q = bobs_off[b]; q < bobs_off[b + 1]; ++q) {
            const int cf = d_cf[bobs[q]];
            if (cf_pc[cf] == 0) continue;
            tiles.insert(cf_roff[cf] / TILE);
            tiles.insert((cf_roff[cf] + cf_pc[cf] - 1) / TILE);
        }
        for (int I : tiles)
            for (int J : tiles)
                if (J <= I) nz[(size_t)I * NT + J] = 1;
    }
    // symbolic fill-in
    panel_rows_off.assign(NT + 1, 0);
    panel_rows.clear();
    std::vector<int2> pairs;
    panel_pairs_off.assign(NT + 1, 0);
    for (int k = 0; k < NT; ++k) {
        std::vector<int> rows;
        for (int I = k + 1; I < NT; ++I)
            if (nz[(size_t)I * NT + k]) rows.push_back(I);
        for (size_t a = 0; a < rows.size(); ++a)
            for (size_t c = 0; c <= a; ++c) nz[(size_t)rows[a] * NT + rows[c]] = 1;
        panel_rows_off[k] = (int)panel_rows.size();
        for (int I : rows) panel_rows.push_back(I);
        panel_pairs_off[k] = (int)pairs.size();
        for (size_t a = 0; a < rows.size(); ++a)
            for (size_t c = 0; c <= a; ++c) pairs.push_back(make_int2(rows[a], rows[c]));
    }
    panel_rows_off[NT] = (int)panel_rows.size();
    panel_pairs_off[NT] = (int)pairs.size();
    panel_cols_off.assign(NT + 1, 0);
    panel_cols.clear();
    for (int k = 0; k < NT; ++k) {
        panel_cols_off[k] = (int)panel_cols.size();
        for (int J = 0; J < k; ++J)
            if (nz[(size_t)k * NT + J]) panel_cols.push_back(J);
    }
    panel_cols_off[NT] = (int)panel_cols.size();
    std::vector<int> slot((size_t)NT * NT, -1);
    nslots = 0;
    for (int I = 0; I < NT; ++I)
        for (int J = 0; J <= I; ++J)
            if (nz[(size_t)I * NT + J]) slot[(size_t)I * NT + J] = nslots++;

    pc_uniform = 0;
    for (int cf = 0; cf < ncf; ++cf) {
        if (cf_pc[cf] == 0) continue;
        if (pc_uniform == 0) pc_uniform = cf_pc[cf];
        else if (pc_uniform != cf_pc[cf]) pc_uniform = -1;
    }
    if (pc_uniform < 0) pc_uniform = 0;
    // ---- Schur accumulation plan: observation pairs sharing a bundle, sorted
    // by destination block (cf_i >= cf_j) ----
    std::vector<int2> dest_h, dpairs_h;
    std::vector<int> dest_off_h;
    {
        long long npairs = 0;
        for (int b = 0; b < nB; ++b)
            if (bnd_pb[b] > 0) {
                const long long kb = rs_bnd ? vbobs_off[b + 1] - vbobs_off[b] : bobs_off[b + 1] - bobs_off[b];
                npairs += kb * kb;
            }
        use_dest = nB_solved > 0 && nR > 0 && npairs <= (1ll << 30);
        if (nranks > 1 && nB_solved > 0 && !use_dest)
            throw Unsupported{"sharded solve: too many observation pairs per bundle"};
        if (use_dest) {
            struct PairRec {
                int cfi, cfj, i, j;
            };
            // bucket by destination row cfi (counting pass), then sort each
            // bucket by (cfj, i, j): O(pairs) grouping instead of one global
            // sort (C3: ~50M pairs)
            std::vector<long long> cnt(ncf + 1, 0);
            // (rolling shutter with solved bundles: the virtual observations)
            const std::vector<int> &sbo = rs_bnd ? vbobs_off : bobs_off;
            const std::vector<int> &sb = rs_bnd ? vbobs : bobs;
            const std::vector<int> &scf = rs_bnd ? v_cf : d_cf;
            auto for_pairs = [&](auto &&fn) {
                for (int b = 0; b < nB; ++b) {
                    if (bnd_pb[b] == 0) continue;
                    for (int qi = sbo[b]; qi < sbo[b + 1]; ++qi) {
                        const int i = sb[qi], cfi = scf[i];
                        if (cf_pc[cfi] == 0 || !cf_own[cfi]) continue;
                        for (int qj = sbo[b]; qj < sbo[b + 1]; ++qj) {
                            const int j = sb[qj], cfj = scf[j];
                            // destination rows must be this shard's camera-frames
                            if (cf_pc[cfj] == 0 || cfi < cfj) continue;
                            fn(cfi, cfj, i, j);
                        }
                    }
                }
            };
            for_pairs([&](int cfi, int, int, int) { cnt[cfi + 1]++; });
            for (int cf = 0; cf < ncf; ++cf) cnt[cf + 1] += cnt[cf];
            std::vector<PairRec> recs((size_t)cnt[ncf]);
            {
                std::vector<long long> pos(cnt.begin(), cnt.end() - 1);
                for_pairs([&](int cfi, int cfj, int i, int j) { recs[pos[cfi]++] = {cfi, cfj, i, j}; });
            }
            for (int cf = 0; cf < ncf; ++cf)
                std::sort(recs.begin() + cnt[cf], recs.begin() + cnt[cf + 1],
                          [](const PairRec &x, const PairRec &y) {
                              if (x.cfj != y.cfj) return x.cfj < y.cfj;
                              if (x.i != y.i) return x.i < y.i;
                              return x.j < y.j;
                          });
            dpairs_h.reserve(recs.size());
            for (size_t q = 0; q < recs.size(); ++q) {
                if (q == 0 || recs[q].cfi != recs[q - 1].cfi || recs[q].cfj != recs[q - 1].cfj) {
                    dest_h.push_back(make_int2(recs[q].cfi, recs[q].cfj));
                    dest_off_h.push_back((int)q);
                }
                dpairs_h.push_back(make_int2(recs[q].i, recs[q].j));
            }
            dest_off_h.push_back((int)recs.size());
            ndest = (int)dest_h.size();
            // k_schur_init folds into the diagonal destinations when every
            // solved camera-frame has one (its rows are then all written)
            std::vector<char> hasd(ncf, 0);
            for (const int2 &d : dest_h)
                if (d.x == d.y) hasd[d.x] = 1;
            dest_diag_all = true;
            for (int cf = 0; cf < ncf; ++cf)  // (sharded: this shard's camera-frames)
                if (cf_pc[cf] > 0 && cf_own[cf] && !hasd[cf]) dest_diag_all = false;
            dest_diag_ii = true;
            for (size_t d = 0; d < dest_h.size() && dest_diag_ii; ++d)
                if (dest_h[d].x == dest_h[d].y)
                    for (int q = dest_off_h[d]; q < dest_off_h[d + 1]; ++q)
                        if (dpairs_h[q].x != dpairs_h[q].y) {
                            dest_diag_ii = false;
                            break;
                        }
        }
    }
    {
        int widest = 0;
        for (int k = 0; k < NT; ++k) {
            widest = std::max(widest, panel_rows_off[k + 1] - panel_rows_off[k]);
            widest = std::max(widest, panel_cols_off[k + 1] - panel_cols_off[k]);
        }
        narrow = NT > 0 && widest <= 8;
    }

    // ---- device upload ----
    size_t nvals = 0;
    for (int a = 0; a < nA; ++a)
        nvals = std::max(nvals, (size_t)pr->attr_offset[a] + (pr->attr_animated[a] ? F : 1));
    host_attr0.assign(pr->attr_values, pr->attr_values + nvals);
    attr_bytes = nvals * sizeof(double);

    DevProblem D{};
    D.F = F;
    D.nA = nA;
    D.nT = nT;
    D.nC = nC;
    D.nL = nL;
    D.nB = nB;
    D.nK = nK;
    D.M = M;
    D.n = n;
    D.ncf = ncf;
    D.nR = nR;
    D.nG = nG;
    D.mode = opt.scene_graph_mode;
    D.image_width = opt.image_width;
    D.attr_off = upload(pr->attr_offset, nA);
    D.attr_anim = upload(pr->attr_animated, nA);
    d_attr0 = upload(host_attr0);
    D.attr_val = dalloc<double>(nvals);
    D.tfm_parent = upload(pr->tfm_parent, nT);
    D.tfm_roo = upload(pr->tfm_rotate_order, nT);
    D.tfm_attrs = upload(pr->tfm_attrs, 9 * (size_t)nT);
    D.cam_tfm = upload(pr->cam_tfm, nC);
    D.cam_attrs = upload(pr->cam_attrs, MMBA_CAM_NUM_ATTRS * (size_t)nC);
    D.cam_fit = upload(pr->cam_film_fit, nC);
    D.cam_size = upload(pr->cam_render_size, 2 * (size_t)nC);
    D.cam_lens = pr->cam_lens ? upload(pr->cam_lens, nC) : nullptr;
    D.lens_attrs = upload(pr->lens_attrs, MMBA_LENS_NUM_ATTRS * (size_t)nL);
    D.lens_type = upload(pr->lens_type, nL);
    D.lens_chain = lens_chain_h.empty() ? nullptr : upload(lens_chain_h);
    D.lens_chain_n = (int)(lens_chain_h.size() / LENS_LAYER);
    {
        // the one lens model every instance uses (k_jacobian's fixed-model form)
        int lt = -2;
        for (int l : inst_lens_h) {
            const int t = pr->lens_type[l];
            lt = (lt == -2 || lt == t) ? t : -1;
        }
        D.lens_uniform = (D.lens_chain_n == 0 && lt >= 0) ? lt : -1;
    }
    D.bnd_tfm = upload(pr->bnd_tfm, nB);
    D.obs_cf = upload(d_cf);
    D.obs_bnd = upload(d_bnd);
    D.obs_frame = upload(d_frame);
    D.obs_cam = upload(d_cam);
    D.obs_xy = d_obs_xy = upload(d_xy);
    D.obs_sqrtw = d_obs_sqrtw = upload(d_sqrtw);
    if (!obs_xy_src.empty()) {
        std::vector<int> src(M);
        for (int i = 0; i < M; ++i) src[i] = obs_xy_src[ref_of_dev[i]];
        d_xy_src = upload(src);
    }
    setup_marker_refresh(nK);
    D.cf_cam = upload(cf_cam);
    D.cf_frame = upload(cf_frame);
    D.cf_obs_off = upload(cf_obs_off);
    D.cf_var_off = upload(cf_var_off);
    D.cf_var_param = upload(cf_var_param);
    D.cf_var_flags = upload(cf_var_flags);
    D.cf_pc = upload(cf_pc);
    D.cf_roff = upload(cf_roff);
    D.pc_uniform = pc_uniform;
    D.wst = 3 * (pc_uniform > 0 ? pc_uniform : PCMAX);
    D.bnd_par_off = upload(bnd_par_off);
    D.bnd_par = upload(bnd_par);
    D.bnd_pb = upload(bnd_pb);
    D.bnd_xoff = nullptr;
    D.bnd_p4 = upload(bnd_p4);
    {
        // per-camera-frame attribute-value indices for the camera records
        // (cameras whose transform has no parent; in rolling-shutter plans
        // every camera: the records then multiply by the parent's world
        // matrix, camera_record_fast / rs_record)
        bool ok = true;
        for (int c = 0; c < nC && ok && !rs_on; ++c)
            if (pr->tfm_parent[pr->cam_tfm[c]] >= 0) ok = false;
        D.cf_aidx = nullptr;
        if (ok && ncf > 0) {
            static const int cam_k[7] = {MMBA_CAM_FILM_BACK_W_INCH, MMBA_CAM_FILM_BACK_H_INCH,
                                         MMBA_CAM_FILM_OFFSET_X_INCH, MMBA_CAM_FILM_OFFSET_Y_INCH,
                                         MMBA_CAM_FOCAL_MM, MMBA_CAM_FAR_CLIP, MMBA_CAM_SCALE};
            std::vector<int> tab((size_t)CF_AIDX * ncf, -1);
            auto vidx = [&](int a, int f) -> int {
                if (a < 0) return -1;
                const long long ix = pr->attr_offset[a] + (pr->attr_animated[a] ? f : 0);
                if (ix > INT32_MAX) throw Unsupported{"attribute block over 2^31 values"};
                return (int)ix;
            };
            for (int cf = 0; cf < ncf; ++cf) {
                const int c = cf_cam[cf], f = cf_frame[cf];
                for (int k = 0; k < 7; ++k)
                    tab[(size_t)CF_AIDX * cf + k] =
                        vidx(pr->cam_attrs[MMBA_CAM_NUM_ATTRS * c + cam_k[k]], f);
                const int t = pr->cam_tfm[c];
                for (int k = 0; k < 9; ++k)
                    tab[(size_t)CF_AIDX * cf + 7 + k] = vidx(pr->tfm_attrs[9 * t + k], f);
            }
            D.cf_aidx = upload(tab);
        }
    }
    D.nbs = nB_solved;
    D.dest_diag_ii = dest_diag_ii ? 1 : 0;
    D.all_bnd_fast = 1;
    for (int b = 0; b < nB; ++b)
        if (bnd_p4[b].w < 0) D.all_bnd_fast = 0;
    D.no_lens = 1;
    for (int c = 0; c < nC; ++c)
        if (pr->cam_lens && pr->cam_lens[c] >= 0) D.no_lens = 0;
    {
        std::vector<int> bpos(M);
        for (int q = 0; q < M; ++q) bpos[bobs[q]] = q;
        D.obs_bpos = upload(bpos);
        // (the rolling-shutter Jacobian writes no bundle block records: its
        // bundle normal equations come from the J rows, k_ne_bnd)
        bool all_fast = nG == 0 && nB_solved > 0 && !rs_on;
        for (int b = 0; b < nB && all_fast; ++b)
            if (bnd_pb[b] > 0 && bnd_p4[b].w < 0) all_fast = false;
        D.JB = all_fast ? dalloc<double>((size_t)8 * M) : nullptr;
        // uniform fast Jacobian kernel: fast bundles, no lens, no bundle-side
        // camera variants, at most pc_uniform (6 or 7) variants per camera-frame
        bool fast = nG == 0 && (pc_uniform == 6 || pc_uniform == 7);
        for (int b = 0; b < nB && fast; ++b)
            if (bnd_pb[b] > 0 && bnd_p4[b].w < 0) fast = false;
        for (int c = 0; c < nC && fast; ++c)
            if (pr->cam_lens && pr->cam_lens[c] >= 0) fast = false;
        for (size_t t = 0; t < cf_var_flags.size() && fast; ++t)
            if (cf_var_flags[t] != 0) fast = false;
        for (int cf = 0; cf < ncf && fast; ++cf)
            if (cf_var_off[cf + 1] - cf_var_off[cf] - 1 > pc_uniform) fast = false;
        // central differences, the robust loss and the rolling shutter run on
        // the generic kernels
        if (central || opt.robust_loss || rs_on) fast = false;
        jac_ncv = fast ? pc_uniform : 0;
        D.jcol_implicit = jac_ncv > 0 ? 1 : 0;
    }
    d_brec = dalloc<double>((size_t)nB * BREC);
    D.brec = d_brec;
    D.bobs_off = upload(bobs_off);
    D.bobs = upload(bobs);
    {
        std::vector<int2> rp(M);
        for (int q = 0; q < M; ++q) {
            const int cf = d_cf[bobs[q]];
            rp[q] = make_int2(cf_roff[cf], cf_pc[cf]);
        }
        d_bobs_rp = upload(rp);
    }
    {
        // k_schur_obs's per-observation word (MMBA_PATH_LOADS_FIRST)
        std::vector<int> sp(M);
        bool fits = true;  // (a camera-frame with more variants keeps the table walk)
        for (int i = 0; i < M; ++i) {
            const int cf = d_cf[i];
            const int sv = cf_var_off[cf + 1] - cf_var_off[cf] - 1;
            fits = fits && sv >= 0 && sv < 256;
            sp[i] = sv | (cf_pc[cf] << 8) | (bnd_pb[d_bnd[i]] << 16);
        }
        D.obs_sp = fits ? upload(sp) : nullptr;
    }
    D.cam_lpar_off = upload(cam_lpar_off);
    {
        bool any_inst = false;
        for (int i = 0; i < M; ++i) any_inst |= d_inst[i] >= 0;
        if (any_inst) {
            D.obs_inst = upload(d_inst);
            D.inst_lens = upload(inst_lens_h);
            D.inst_attr = upload(inst_attr_h);
            D.inst_frame = upload(inst_frame_h);
            D.inst_val = upload(inst_val_h);
            D.inst_lpar_off = upload(inst_lpar_off_h);
            D.inst_lpar = upload(inst_lpar_h.empty() ? std::vector<int>{-1} : inst_lpar_h);
            d_inst_attr_plug = upload(std::vector<int>(inst_attr_h.size(), -1));
        } else {
            D.obs_inst = nullptr;
        }
    }
    D.cam_lpar = upload(cam_lpar);
    {
        // widest observation (local Jacobian columns): camera variants +
        // bundle-side parameters + the camera's lens parameters
        int lm = 1;
        for (int i = 0; i < M; ++i) lm = std::max(lm, obs_cols(i));
        D.lmax = std::min(lm, LMAX);
    }
    D.p_attr = upload(pr->param_attr, n);
    D.p_frame = upload(pr->param_frame, n);
    D.p_class = upload(p_class);
    D.p_pos = upload(p_pos);
    D.p_both = upload(p_both);
    D.p_blk = upload(p_blk);
    D.p_min = upload(pr->param_min, n);
    D.p_max = upload(pr->param_max, n);
    D.p_off = upload(pr->param_offset, n);
    D.p_scale = upload(pr->param_scale, n);
    D.g_param = upload(g_param);
    D.root = rank == 0 ? 1 : 0;
    D.Ra = Ra;
    D.Rb = Rb;
    D.nrows = nrows;
    D.rows_live = opt.scene_graph_mode == MMBA_SCENE_GRAPH_MM_SCENE_GRAPH ? 0 : 1;
    D.row_attr = upload(row_attr);
    D.row_frame = upload(row_frame);
    D.row_param = upload(row_param);
    D.row_w = upload(row_w);
    D.row_var = upload(row_var);
    D.row_val = upload(row_val);
    D.p_vidx = upload(param_vidx);
    D.bnd_vx = nullptr;
    D.bnd_pcomp = nullptr;
    {
        // fast parentless bundles: value indices of the translate and the
        // component each parameter sets
        bool ok = nB > 0;
        bool fwd = true;  // brec_fwd: each parameter sets its own, distinct component
        std::vector<int4> vx(std::max(nB, 1), make_int4(-1, -1, -1, 0));
        std::vector<int> pcomp(std::max(nB, 1), 0);
        for (int b = 0; b < nB && ok; ++b) {
            const int t = pr->bnd_tfm[b];
            if (pr->tfm_parent[t] >= 0) {
                ok = false;
                break;
            }
            int ix[3];
            for (int k = 0; k < 3; ++k) {
                const int a = pr->tfm_attrs[9 * t + k];
                if (a >= 0 && pr->attr_animated[a]) ok = false;
                const long long v = a < 0 ? -1 : (long long)pr->attr_offset[a];
                if (v > INT32_MAX) ok = false;
                ix[k] = (int)v;
            }
            vx[b] = make_int4(ix[0], ix[1], ix[2], 0);
            const int4 p4 = bnd_p4[b];
            if (p4.w < 0) continue;  // generic bundle: not read through the table
            const int ps[3] = {p4.x, p4.y, p4.z};
            int seen = 0;
            for (int a = 0; a < p4.w && ok; ++a) {
                const int pa = pr->param_attr[ps[a]];
                int comp = -1;
                for (int k = 0; k < 3; ++k)
                    if (pr->tfm_attrs[9 * t + k] == pa) comp = k;
                if (comp < 0) {
                    ok = false;
                } else {
                    pcomp[b] |= comp << (2 * a);
                    if ((seen >> comp) & 1 || param_vidx[ps[a]] != (long long)ix[comp])
                        fwd = false;
                    seen |= 1 << comp;
                }
            }
        }
        if (ok) {
            D.bnd_vx = upload(vx);
            D.bnd_pcomp = upload(pcomp);
        }
        brec_fwd = ok && fwd;
    }
    D.rs = rs_on ? 1 : 0;
    D.obs_tau = nullptr;
    D.cf_rs_nb = nullptr;
    D.cf_rs_vidx = nullptr;
    D.cf_rs_gcnt = D.cf_rs_gcol = D.cf_rs_gidx = nullptr;
    D.rs_Aoff = nullptr;
    if (rs_on) {
        if (!D.cf_aidx) throw Unsupported{"rolling shutter needs the camera-frame table"};
        std::vector<double> tau(M), obs_rs(M);
        for (int i = 0; i < M; ++i) {
            const int r = ref_of_dev[i];
            obs_rs[i] = pr->cam_rs_value[d_cam[i]];
            tau[i] = pr->cam_rs_value[d_cam[i]] * (0.5 - pr->obs_xy[2 * r + 1]);
        }
        D.obs_tau = d_obs_tau = upload(tau);
        d_obs_rs = upload(obs_rs);  // k_marker_set recomputes tau from it
        D.cf_rs_nb = upload(cf_nb);
        std::vector<int> vx((size_t)12 * ncf, -1);
        for (int cf = 0; cf < ncf; ++cf) {
            const int c = cf_cam[cf], f = cf_frame[cf], t = pr->cam_tfm[c];
            for (int k = 0; k < 6; ++k) {
                const int a = pr->tfm_attrs[9 * t + k];
                auto vi = [&](int fr) -> int {
                    if (fr < 0 || fr >= F) return -2;  // the exporter's extrapolation
                    if (a < 0) return -1;
                    return (int)(pr->attr_offset[a] + (pr->attr_animated[a] ? fr : 0));
                };
                vx[(size_t)12 * cf + k] = vi(f - 1);
                vx[(size_t)12 * cf + 6 + k] = vi(f + 1);
            }
        }
        D.cf_rs_vidx = upload(vx);
        // the global columns of each segment's rows, in k_jacobian_rs's
        // column order: variants (CF params, camera-side globals), the
        // neighbours' CF params, the lens params reaching the frame
        std::vector<int> gcnt(std::max(ncf, 1), 0), gcol((size_t)NGMAX * std::max(ncf, 1), -1),
            gidx((size_t)NGMAX * std::max(ncf, 1), -1);
        for (int cf = 0; cf < ncf; ++cf) {
            std::vector<int> cols;
            for (int v = cf_var_off[cf] + 1; v < cf_var_off[cf + 1]; ++v) cols.push_back(cf_var_param[v]);
            for (int side = 0; side < 2; ++side) {
                const int cn = cf_nb[2 * cf + side];
                if (cn >= 0)
                    for (int p : cf_params[cn]) cols.push_back(p);
            }
            // the segment's lens columns: k_jacobian_rs reduces the
            // segment's rows into one block, so they must be the same
            // parameters for every observation of the segment, and (the
            // blend re-measures the neighbouring frames too) each one static
            // or keyed at the segment's own frame
            const int j0 = cf_obs_off[cf] < cf_obs_off[cf + 1] ? d_inst[cf_obs_off[cf]] : -1;
            for (int i = cf_obs_off[cf]; i < cf_obs_off[cf + 1]; ++i) {
                const int j = d_inst[i];
                const int n0 = j0 < 0 ? 0 : inst_lpar_off_h[j0 + 1] - inst_lpar_off_h[j0];
                const int n1 = j < 0 ? 0 : inst_lpar_off_h[j + 1] - inst_lpar_off_h[j];
                bool same = n0 == n1;
                for (int q = 0; q < n0 && same; ++q)
                    same = inst_lpar_h[inst_lpar_off_h[j0] + q] == inst_lpar_h[inst_lpar_off_h[j] + q];
                if (!same)
                    throw Unsupported{"rolling shutter where the observations of one camera-frame "
                                      "read lens instances with different parameters (B3)"};
            }
            if (j0 >= 0)
                for (int q = inst_lpar_off_h[j0]; q < inst_lpar_off_h[j0 + 1]; ++q) {
                    const int p = inst_lpar_h[q];
                    if (pr->param_frame[p] >= 0 && pr->param_frame[p] != cf_frame[cf])
                        throw Unsupported{"rolling shutter where a camera-frame's lens instance "
                                          "holds another frame's animated lens parameter (B3)"};
                    cols.push_back(p);
                }
            for (int l = 0; l < (int)cols.size() && l < LMAX; ++l)
                if (p_class[cols[l]] == PC_G && gcnt[cf] < NGMAX) {
                    gcol[(size_t)NGMAX * cf + gcnt[cf]] = l;
                    gidx[(size_t)NGMAX * cf + gcnt[cf]] = p_pos[cols[l]] - nCF;
                    ++gcnt[cf];
                }
        }
        D.cf_rs_gcnt = upload(gcnt);
        D.cf_rs_gcol = upload(gcol);
        D.cf_rs_gidx = upload(gidx);
        D.rs_Aoff = dalloc<double>((size_t)2 * ncf * PCMAX * PCMAX);
        MMBA_HIP(hipMemsetAsync(D.rs_Aoff, 0, sizeof(double) * 2 * ncf * PCMAX * PCMAX, s));
    }
    D.ls_ng = (int)ls_host.size();
    D.ls_nl = (int)ls_link_cf.size();
    D.ls_tab = nullptr;
    D.ls_Aoff = nullptr;
    if (D.ls_ng > 0) {
        std::vector<int> tab;
        for (const std::vector<int> *v :
             {&ls_host, &ls_nh, &ls_link_off, &ls_hpar, &ls_hpos, &ls_link_cf, &ls_link_grp})
            tab.insert(tab.end(), v->begin(), v->end());
        D.ls_tab = upload(tab);
        D.ls_Aoff = dalloc<double>((size_t)D.ls_nl * PCMAX * PCMAX);
        MMBA_HIP(hipMemsetAsync(D.ls_Aoff, 0, sizeof(double) * D.ls_nl * PCMAX * PCMAX, s));
    }
    // object records (mmba_object.hip): the world matrix of every bundle
    // parent whose chain an animated or solved attribute moves, once per
    // evaluation and frame instead of once per observation and column.  Where
    // the generic kernels run (k_jacobian / k_residual; the uniform kernels
    // keep the chain walk), forward differences, no rolling shutter, one device
    orec = ObjRecDev();
    obj_rec_moved = false;
    const int rec_pin = path_choice(MMBA_PATH_OBJ_REC);
    if ((rec_pin < 0 ? kObjRecDefault : rec_pin != 0) && !rs_on && !central && nranks == 1 &&
        jac_ncv == 0) {
        std::vector<std::vector<int>> attr_params(nA);
        for (int p = 0; p < n; ++p) attr_params[pr->param_attr[p]].push_back(p);
        // the parameters of each transform's chain (ascending), and whether
        // anything moves the chain at all
        std::vector<int> moves(nT, -1);
        auto chain_moves = [&](int t) -> bool {
            if (moves[t] < 0) {
                moves[t] = 0;
                for (int u : chain[t])
                    for (int k = 0; k < 9; ++k) {
                        const int a = pr->tfm_attrs[9 * u + k];
                        if (a >= 0 && (pr->attr_animated[a] || !attr_params[a].empty())) moves[t] = 1;
                    }
            }
            return moves[t] == 1;
        };
        std::map<std::pair<int, int>, int> set_id;
        std::vector<int> obs_orec(M, -1), tf;
        for (int i = 0; i < M; ++i) {
            const int b = d_bnd[i];
            const int t = pr->tfm_parent[pr->bnd_tfm[b]];
            if (bnd_p4[b].w >= 0 || t < 0 || !chain_moves(t)) continue;
            auto ins = set_id.emplace(std::make_pair(t, d_frame[i]), (int)set_id.size());
            if (ins.second) {
                tf.push_back(t);
                tf.push_back(d_frame[i]);
            }
            obs_orec[i] = ins.first->second;
        }
        const int nset = (int)set_id.size();
        if (nset > 0) {
            std::vector<int> off(nset + 1, 0), par, set;
            for (int r = 0; r < nset; ++r) {
                off[r] = (int)par.size();
                par.push_back(-1);
                set.push_back(r);
                std::set<int> ps;
                for (int u : chain[tf[2 * r]])
                    for (int k = 0; k < 9; ++k) {
                        const int a = pr->tfm_attrs[9 * u + k];
                        if (a < 0) continue;
                        for (int p : attr_params[a])
                            if (pr->param_frame[p] < 0 || pr->param_frame[p] == tf[2 * r + 1])
                                ps.insert(p);
                    }
                for (int p : ps) {
                    par.push_back(p);
                    set.push_back(r);
                }
            }
            off[nset] = (int)par.size();
            obj_rec_moved = (int)par.size() > nset;
            orec.n = (int)par.size();
            orec.obs_set = upload(obs_orec);
            orec.off = upload(off);
            orec.par = upload(par);
            orec.set = upload(set);
            orec.tf = upload(tf);
            orec.rec = dalloc<double>((size_t)orec.n * ORECSZ);
        }
    }
    D.loss_on = opt.robust_loss ? 1 : 0;
    D.loss_type = opt.robust_loss_type;
    D.loss_scale = opt.robust_loss_scale;
    p_own.assign(n, 1);
    if (nranks > 1) {
        std::vector<int> bown(nB);
        for (int b = 0; b < nB; ++b) bown[b] = bnd_owner[b] == rank ? 1 : 0;
        for (int q = 0; q < n; ++q) {
            if (p_class[q] == PC_CF) p_own[q] = cf_own[p_blk[q]];
            else if (p_class[q] == PC_B) p_own[q] = bown[p_blk[q]];
            else p_own[q] = rank == 0 ? 1 : 0;
        }
        // every parameter's owner, the same rule for every rank
        for (int q = 0; q < n; ++q)
            obs_rank_g[(size_t)Mg + q] = p_class[q] == PC_CF  ? cf_rank[p_blk[q]]
                                         : p_class[q] == PC_B ? bnd_owner[p_blk[q]]
                                                              : 0;
        D.obs_own = upload(d_own);
        D.cf_own = upload(cf_own);
        D.bnd_own = upload(bown);
        d_p_own = upload(p_own);
    }
    p_class_h = p_class;
    p_blk_h = p_blk;
    P = D;
    if (rs_bnd) {
        PV = P;
        PV.M = Mv;
        PV.obs_cf = upload(v_cf);
        PV.obs_bnd = upload(v_bnd);
        PV.cf_obs_off = upload(vcf_off);
        PV.bobs_off = upload(vbobs_off);
        PV.bobs = upload(vbobs);
        d_vobs = upload(v_obs);
        d_vcoff = upload(v_coff);
    }

    d_var_cf = upload(var_cf);
    d_stale = upload(stale);
    d_ref_of_dev = upload(ref_of_dev);
    {  // deviation metrics: this shard's own observations, keyed as the caller keys them
        std::vector<int> dev_of_own(Mg, -1);
        for (int i = 0; i < M; ++i)
            if (obs_own_g[ref_of_dev[i]]) dev_of_own[ref_of_dev[i]] = i;
        setup_metrics(F, nK, Mg, pr->obs_marker, pr->obs_frame, dev_of_own);
    }
    if (nranks == 1 && M > 0) {  // the host-mapped hand-back gathers in reference order
        std::vector<int> dev_of_ref(M, 0);
        for (int i = 0; i < M; ++i) dev_of_ref[ref_of_dev[i]] = i;
        d_dev_of_ref = upload(dev_of_ref);
    }
    d_slot = upload(slot);
    d_rows = upload(panel_rows);
    d_cols = upload(panel_cols);
    d_pairs = upload(pairs);
    d_rows_off = upload(panel_rows_off);
    d_cols_off = upload(panel_cols_off);
    if (use_dest) {
        d_dest = upload(dest_h);
        d_dest_off = upload(dest_off_h);
        d_dpairs = upload(dpairs_h);
        // many small off-diagonal destinations (C3: 9.3M destinations of 5.5
        // pairs on average): those of at most 32 pairs take one lane each
        // (k_schur_dest_lane, the same sums in the same order), the others
        // (diagonal ones among them) a wave each
        if (pc_uniform == 6 || pc_uniform == 7) {
            std::vector<int> wl, ll;
            for (int d = 0; d < ndest; ++d) {
                const bool lane = dest_h[d].x != dest_h[d].y && dest_off_h[d + 1] - dest_off_h[d] <= 32;
                (lane ? ll : wl).push_back(d);
            }
            const int pin = path_choice(MMBA_PATH_DEST_LANE);  // 1: whenever there are any
            if (!ll.empty() && pin != 0 &&
                (pin == 1 || (ll.size() >= 16384 && 2 * ll.size() >= (size_t)ndest))) {
                n_dest_wave = (int)wl.size();
                n_dest_lane = (int)ll.size();
                d_dest_wave = upload(wl.empty() ? std::vector<int>(1, 0) : wl);
                d_dest_lane = upload(ll);
            }
        }
    }
    {
        // dense reduced system: at least 30 % of the lower tiles non-zero
        // after fill (MMBA_PATH_DENSE pins it: 0 tiled, 1 dense)
        const long long full = (long long)NT * (NT + 1) / 2;
        dense = !band && nranks == 1 && NT >= 8 && (long long)nslots * 10 >= full * 3;
        if (path_choice(MMBA_PATH_DENSE) >= 0)
            dense = !band && nranks == 1 && NT > 0 && path_choice(MMBA_PATH_DENSE) != 0;
        if (shard_dense) dense = true;  // sharded, not a band: the dense solver (above)
    }
    if (dense) {
        ds.setup(*this, nRpad);
        d_S = ds.A;
        dld = ds.ld;
        d_Linv = nullptr;
        // sharded: every shard factors the same all-reduced S, so the rows
        // of lmpar's L^-1 w are counted on shard 0 only
        if (nranks > 1) d_ymask = upload(std::vector<int>(std::max(nR, 1), rank == 0 ? 1 : 0));
    } else {
        d_S = dalloc<double>((size_t)nslots * TILE * TILE);
        d_Linv = dalloc<double>((size_t)NT * TILE * TILE);
    }
    cfblk_roff.clear();
    cfblk_pc.clear();
    cfblk_cf.clear();
    for (int cf = 0; cf < ncf; ++cf)
        if (cf_pc[cf] > 0) {
            cfblk_roff.push_back(cf_roff[cf]);
            cfblk_pc.push_back(cf_pc[cf]);
            cfblk_cf.push_back(cf);
        }
    if (band) setup_band();
    if (path_choice(MMBA_PATH_PROBE) == 2) {  // k_jac_ne_u workgroup timeline
        const size_t np = K2_PROBE_N * (size_t)std::max(ncf, 1);
        d_k2probe = dalloc<long long>(np);
        MMBA_HIP(hipMemsetAsync(d_k2probe, 0, np * sizeof(long long), s));
    }
    if (band && path_choice(MMBA_PATH_PROBE) == 1) {
        const size_t np = 8 + 4 * ((size_t)std::max(nR, 1) + 64);  // + the dataflow trace
        d_probe = dalloc<long long>(np);
        MMBA_HIP(hipMemsetAsync(d_probe, 0, np * sizeof(long long), s));
    }

    d_x = dalloc<double>(n);
    d_ext = dalloc<double>(n);
    d_ext_pert = dalloc<double>(n);
    d_step = dalloc<double>(n);
    d_diag = dalloc<double>(n);
    d_acnorm = dalloc<double>(n);
    d_g = dalloc<double>(n);
    d_wa1 = dalloc<double>(n);
    d_wa2 = dalloc<double>(n);
    d_wa3 = dalloc<double>(n);
    d_xs = dalloc<double>(n);
    d_v = dalloc<double>(n);
    d_f = dalloc<double>(m);
    d_ftrial = dalloc<double>(m);
    d_eu = dalloc<double>(m);
    d_ed = dalloc<double>(M);
    d_eu_s = dalloc<double>(m);
    d_ed_s = dalloc<double>(M);
    for (double *b : {d_f, d_ftrial, d_eu, d_eu_s})
        MMBA_HIP(hipMemsetAsync(b, 0, sizeof(double) * m, s));
    d_Jrow = dalloc<double>(nrows);
    d_dist_x = dalloc<double>(M);
    d_dist_t = dalloc<double>(M);
    d_recs = dalloc<double>((size_t)nvar * CAMREC);
    if (central) {
        d_ext_pertB = dalloc<double>(n);
        d_stepB = dalloc<double>(n);
        d_recsB = dalloc<double>((size_t)nvar * CAMREC);
        d_brecB = dalloc<double>((size_t)nB * BREC);
    }
    if (b15) {
        d_c15 = dalloc<double>(n);
        d_c15r = dalloc<double>(n);
        d_g15 = dalloc<double>(n);
        d_z15u = dalloc<double>(n);
        d_z15c = dalloc<double>(n);
        d_q15 = dalloc<double>((size_t)ncf * PCMAX * PCMAX);
        d_kap15 = dalloc<double>(ncf);
        d_AccL = dalloc<double>((size_t)ncf * PCMAX * PCMAX);
        d_diagL = dalloc<double>(n);
        d_xs15r = dalloc<double>(n);
        d_p15 = dalloc<double>(n);
        d_v15 = dalloc<double>(n);
        d_adiag15 = dalloc<double>(n);
        d_u15 = dalloc<double>(n);
        d_b15k = dalloc<double>(8);
        MMBA_HIP(hipMemsetAsync(d_b15k, 0, sizeof(double) * 8, s));
    }
    // J / jcol: the widest observation's columns (D.lmax <= LMAX), not LMAX
    d_J = dalloc<double>(std::max((size_t)2 * D.lmax * M, (size_t)m + M));
    d_jcol = dalloc<int>((size_t)std::max(D.lmax, 1) * M);
    d_nloc = dalloc<int>(M);
    d_Acc = dalloc<double>((size_t)ncf * PCMAX * PCMAX);
    // k_ne_cf_split's partial sums and per camera-frame tickets (monotonic:
    // zeroed once)
    d_cf_part = dalloc<double>((size_t)std::max(ncf, 1) * NE_CF_SPLIT * NE_CF_NT);
    d_cf_ticket = dalloc<unsigned>((size_t)std::max(ncf, 1));
    MMBA_HIP(hipMemsetAsync(d_cf_ticket, 0, sizeof(unsigned) * std::max(ncf, 1), s));
    d_Acg = dalloc<double>((size_t)ncf * PCMAX * NGMAX);
    d_Abb = dalloc<double>((size_t)nB * 9);
    d_Abg = dalloc<double>((size_t)nB * PBMAX * NGMAX);
    // [Agg | g_G] (launch_ne), then the sharded Jacobian scalars [ZERO, XN2,
    // gnorm of rank 0 .. nranks-1] all-reduced together (Plan::jac)
    d_Agg = dalloc<double>(NGMAX * NGMAX + NGMAX + 2 + std::max(nranks, 1));
    d_gather = dalloc<double>((size_t)2 * mg + Mg + n);
    if (nranks > 1) setup_handback(obs_rank_g);
    d_glob_partial = dalloc<double>((size_t)((M + glob_chunk - 1) / glob_chunk) * (NGMAX * NGMAX + NGMAX));
    d_Lb = dalloc<double>((size_t)nB * 9);
    d_tb = dalloc<double>((size_t)nB * 3);
    d_Wg = dalloc<double>((size_t)nB * NGMAX * 3);
    const int Mw = rs_bnd ? std::max(Mv, 1) : M;  // W rows: (virtual) observations
    d_W = dalloc<double>((size_t)P.wst * (nB_solved > 0 ? Mw : 1));
    d_U = dalloc<double>((size_t)4 * (nB_solved > 0 ? Mw : 1));
    d_rhs = bs.red_rhs ? bs.red_rhs : dalloc<double>(nRpad);
    d_yR = dalloc<double>(nRpad);
    d_xR = dalloc<double>(nRpad);
    d_wR = dalloc<double>(nRpad);
    d_usq = dalloc<double>(nB);
    d_nu = dalloc<double>((size_t)3 * std::max(nB, 1));
    d_ngp = dalloc<double>((size_t)std::max(nG, 1) * std::max(nB, 1));
    pw = std::max(std::max(nparts, residual_blocks(P)), ncf + (nB + NE_BND_TPB - 1) / NE_BND_TPB);
    {
        // parameters outside every solved bundle: the extra workgroups of
        // the fused back substitution + trial pass
        std::vector<char> inb(n, 0);
        for (int b = 0; b < nB; ++b)  // a bundle's own parameters come first (bnd_pb of them)
            for (int a = 0; a < bnd_pb[b]; ++a) inb[bnd_par[bnd_par_off[b] + a]] = 1;
        std::vector<int> other;
        for (int j = 0; j < n; ++j)
            if (!inb[j]) other.push_back(j);
        n_trial_other = (int)other.size();
        d_trial_other = upload(other.empty() ? std::vector<int>(1, 0) : other);
        pw = std::max(pw, trial_fold_parts(P, n_trial_other));
        pw = std::max(pw, trial_fold_parts(P, n_trial_other, true));
        pw = std::max(pw, trial_prep_rec_parts(P, n));  // >= any n_prep_other
    }
    d_partial = dalloc<double>((size_t)8 * pw);  // rows 0..7 (launch_dist_stats: 0..2)
    d_scalar = dalloc<double>(NSLOT);
    d_fail = dalloc<int>(1);
    bs.fail = d_fail;  // the separator form's right-hand-side passes report into it
    if (bs.use_bd) {
        std::vector<int> row_param(std::max(nR, 1), -1);
        for (int p = 0; p < n; ++p)
            if (p_class[p] != PC_B && p_pos[p] >= 0 && p_pos[p] < nR) row_param[p_pos[p]] = p;
        bs.bd.row_param = upload(row_param);
    }
    if (bs.use_bcr && (bs.bcr.flags || bs.use_pcr)) {
        bs.bcr.fail = d_fail;
        if (nranks == 1) {
            std::vector<int> row_param(std::max(nR, 1), -1);
            for (int p = 0; p < n; ++p)
                if (p_class[p] != PC_B && p_pos[p] >= 0 && p_pos[p] < nR) row_param[p_pos[p]] = p;
            bs.bcr.row_param = upload(row_param);
            bs.pcr.row_param = bs.bcr.row_param;
            bs.bcr.xs = bs.bcr.flags ? d_xs : nullptr;
        }
    }
    // ---- batched per-frame solve (mmba_batch.hip): frames share nothing
    // when every parameter belongs to one camera-frame ----
    batch_ok = false;
    {
        const char *why = nullptr;
        // an object-frame parameter left global names what kept it there
        std::string why_obj;
        for (int p = 0; p < n && !why; ++p)
            if (p_class[p] == PC_G && obj_cam[p] != -3) {
                if (obj_off)
                    why_obj = std::string("animated transforms above bundles stay global "
                                          "parameters: ") + obj_off;
                else if (!obj_form)
                    why_obj = "animated transforms above bundles are global parameters of this "
                              "plan (at most " + std::to_string(NGMAX) + " of them): build the "
                              "plan with mmba_plan_create_per_frame";
                else if (obj_cam[p] == -1)
                    why_obj = "an animated transform above bundles seen by several cameras at "
                              "one frame stays a global parameter per frame";
                else
                    why_obj = "an animated transform above bundles at a frame without a "
                              "camera-frame stays a global parameter";
                why = why_obj.c_str();
            }
        for (int p = 0; p < n && !why; ++p)
            if (p_class[p] != PC_CF) why = "a static or shared parameter chains the frames";
        if (!why && nranks != 1) why = "sharded plan";
        for (int p = 0; p < n && !why; ++p)
            if (p_lens[p]) why = "a lens coefficient in a camera-frame block";
        batch_obj = false;
        for (int p = 0; p < n; ++p)
            if (p_obj[p]) batch_obj = true;
        if (!why && nrows > 0) why = "attribute stiffness / smoothness rows";
        if (!why && rs_on) why = "rolling shutter";
        if (!why && (central || opt.robust_loss)) why = "central differences / robust loss";
        std::vector<int> fr_cf_off(F + 1, 0), fr_par_off(F + 1, 0), fr_par, fr_last, fr_nobs;
        int nf = F, nfmax = 0;
        if (!why) {
            for (int cf = 0; cf < ncf; ++cf) fr_cf_off[cf_frame[cf] + 1]++;
            for (int f = 0; f < F; ++f) fr_cf_off[f + 1] += fr_cf_off[f];
            for (int f = 0; f < F && !why; ++f) {
                const int c0 = fr_cf_off[f], c1 = fr_cf_off[f + 1];
                int nl = 0, nobs = 0, last = -1;
                for (int cf = c0; cf < c1; ++cf) {
                    nl += cf_pc[cf];
                    nobs += cf_obs_off[cf + 1] - cf_obs_off[cf];
                }
                if (f < nf && (nl == 0 || nl > 2 * nobs)) nf = f;  // the loop stops here
                if (f >= nf) {
                    fr_par_off[f + 1] = fr_par_off[f];
                    fr_last.push_back(-1);
                    fr_nobs.push_back(nobs);
                    continue;
                }
                if (c1 - c0 > BATCH_CFMAX) why = "more than 8 cameras in one frame";
                if (nl > BATCH_NFMAX) why = "more than 32 parameters in one frame";
                const int r0 = cf_roff[c0];
                for (int k = 0; k < nl; ++k) {
                    int pk = -1;
                    for (int cf = c0; cf < c1 && pk < 0; ++cf)
                        if (r0 + k >= cf_roff[cf] && r0 + k < cf_roff[cf] + cf_pc[cf])
                            pk = cf_params[cf][r0 + k - cf_roff[cf]];
                    fr_par.push_back(pk);
                    last = std::max(last, pk);
                }
                fr_par_off[f + 1] = fr_par_off[f] + nl;
                fr_last.push_back(last);
                fr_nobs.push_back(nobs);
                nfmax = std::max(nfmax, nl);
            }
        }
        // the object form's record slots (BatchObjDev): per solved frame the
        // moving bundle parents its rows hang under -- the rule of the object
        // records above, whether or not that table was built -- base slots
        // first, then a variant per parameter of the frame in a parent's chain
        std::vector<int> fr_slot_off(F + 1, 0), slot_tf, slot_k, slot_set, obs_bset(M, -1);
        if (!why && batch_obj) {
            std::vector<std::vector<int>> attr_params(nA);
            for (int p = 0; p < n; ++p) attr_params[pr->param_attr[p]].push_back(p);
            auto chain_moves = [&](int t) {
                for (int u : chain[t])
                    for (int k = 0; k < 9; ++k) {
                        const int a = pr->tfm_attrs[9 * u + k];
                        if (a >= 0 && (pr->attr_animated[a] || !attr_params[a].empty())) return true;
                    }
                return false;
            };
            std::vector<std::vector<int>> fr_obs(F);
            for (int i = 0; i < M; ++i) fr_obs[d_frame[i]].push_back(i);
            for (int f = 0; f < F && !why; ++f) {
                fr_slot_off[f] = (int)slot_tf.size();
                if (f >= nf) continue;
                std::vector<int> sets;  // transforms, in the rows' order
                for (int i : fr_obs[f]) {
                    const int b = d_bnd[i];
                    const int t = pr->tfm_parent[pr->bnd_tfm[b]];
                    if (bnd_p4[b].w >= 0 || t < 0 || !chain_moves(t)) continue;
                    auto it = std::find(sets.begin(), sets.end(), t);
                    obs_bset[i] = (int)(it - sets.begin());
                    if (it == sets.end()) sets.push_back(t);
                }
                for (size_t q = 0; q < sets.size(); ++q) {
                    slot_tf.push_back(sets[q]);
                    slot_k.push_back(-1);
                    slot_set.push_back((int)q);
                }
                const int k0 = fr_par_off[f], k1 = fr_par_off[f + 1];
                for (size_t q = 0; q < sets.size(); ++q)
                    for (int k = k0; k < k1; ++k) {
                        bool in_chain = false;
                        for (int u : chain[sets[q]])
                            for (int j = 0; j < 9; ++j)
                                in_chain |= pr->tfm_attrs[9 * u + j] == pr->param_attr[fr_par[k]];
                        if (!in_chain) continue;
                        slot_tf.push_back(sets[q]);
                        slot_k.push_back(k - k0);
                        slot_set.push_back((int)q);
                    }
                if ((int)slot_tf.size() - fr_slot_off[f] > BATCH_OSLOTS)
                    why = "more than 32 object records in one frame";
            }
            fr_slot_off[F] = (int)slot_tf.size();
            static_assert(BATCH_OSLOTS == 32, "the refusal's wording");
        }
        if (why) {
            batch_why = why;
        } else {
            batch_ok = true;
            if (batch_obj) {
                bobj.fr_slot_off = upload(fr_slot_off);
                bobj.slot_tf = upload(slot_tf);
                bobj.slot_k = upload(slot_k);
                bobj.slot_set = upload(slot_set);
                bobj.obs_set = upload(obs_bset);
            }
            batch_nf = nf;
            batch_nfmax = nfmax;
            d_fr_cf_off = upload(fr_cf_off);
            d_fr_par_off = upload(fr_par_off);
            d_fr_par = upload(fr_par);
            d_fr_last = upload(fr_last);
            d_fr_nobs = upload(fr_nobs);
        }
    }
    MMBA_HIP(hipMemsetAsync(d_fail, 0, sizeof(int), s));
    // Single-launch reductions (finish_blocks) measured slower than the
    // two-launch form on C4 (the 256-782 arrivals on one ticket plus the
    // release fences cost more than the second launch), so they stay off.
    d_ticket = nullptr;
    MMBA_HIP(hipMemsetAsync(d_Acg, 0, sizeof(double) * (size_t)ncf * PCMAX * NGMAX, s));
    MMBA_HIP(hipMemsetAsync(d_Agg, 0, sizeof(double) * (NGMAX * NGMAX + NGMAX), s));
    MMBA_HIP(hipMemsetAsync(d_Abg, 0, sizeof(double) * (size_t)nB * PBMAX * NGMAX, s));
    MMBA_HIP(hipMemsetAsync(d_Abb, 0, sizeof(double) * (size_t)nB * 9, s));
    MMBA_HIP(hipMemsetAsync(d_Acc, 0, sizeof(double) * (size_t)ncf * PCMAX * PCMAX, s));
    MMBA_HIP(hipHostMalloc(&h_scalar, NSLOT * sizeof(double)));
    MMBA_HIP(hipHostMalloc(&h_seq, sizeof(unsigned)));
    *h_seq = 0;
    trial_fold_ok = nB_solved > 0;
    d_gate = dalloc<int>(1);
    MMBA_HIP(hipMemsetAsync(d_gate, 0, sizeof(int), s));
    d_mticket = dalloc<unsigned>(1);
    d_pweight = upload(param_weight);
    pweight_ok = true;
    for (int j = 0; j < n; ++j)
        if (param_weight[j] <= 0.) pweight_ok = false;
    MMBA_HIP(hipMemsetAsync(d_mticket, 0, sizeof(unsigned), s));
    if (b15) {  // the rank-one term corrects ||J p|| after the trial's reduction
        host_mirror = false;
        trial_fold_ok = false;
    }
    {
        // the trial's records inside its back substitution: every non-bundle
        // parameter is one camera-frame's (its workgroup sets it, then builds
        // that camera-frame's records), at most 15 per camera-frame (16 lanes)
        int maxpc = 0, sumpc = 0;
        for (int cf = 0; cf < ncf; ++cf) {
            maxpc = std::max(maxpc, cf_pc[cf]);
            sumpc += cf_pc[cf];
        }
        trial_rec = trial_fold_ok && nranks == 1 && trial_records_ok(P) && maxpc <= 15 &&
                    sumpc == n_trial_other && nvar == ncf + sumpc &&
                    path_choice(MMBA_PATH_TRIAL_RECORDS) != 0;
        // (a parameter that moves an object record: the trial's records come
        // from the records launch, which rebuilds them)
        if (obj_rec_moved) trial_rec = false;
        // without a solved bundle (C5): the same in k_trial_prep's place, when
        // every parameter outside the camera-frame blocks is a global that no
        // camera or bundle record reads (lens coefficients)
        bool ok = nB_solved == 0 && nranks == 1 && !rs_on && !b15 && P.cf_aidx != nullptr &&
                  ncf > 0 && maxpc <= 15 && nvar == ncf + sumpc &&
                  path_choice(MMBA_PATH_TRIAL_RECORDS) != 0;
        for (int f : cf_var_flags)
            if (f & VF_BUNDLE_SIDE) ok = false;
        // (no parameter moves a bundle: the bundle records stay those of the
        // first evaluation)
        std::vector<int> other;
        for (int p = 0; p < n && ok; ++p) {
            const int a = pr->param_attr[p];
            if (!attr_bnds[a].empty()) ok = false;
            if (p_class[p] == PC_CF) continue;
            if (p_class[p] != PC_G || !attr_cams[a].empty()) ok = false;
            other.push_back(p);
        }
        trial_prep_rec = ok;
        if (ok) {
            n_prep_other = (int)other.size();
            d_prep_other = upload(other.empty() ? std::vector<int>(1, 0) : other);
        }
    }
    fold_init = dest_diag_all && use_dest && nG == 0 && !rs_on && nRpad == nR &&
                (pc_uniform == 6 || pc_uniform == 7);
    MMBA_HIP(hipHostMalloc(&h_fail, sizeof(int)));
    MMBA_HIP(hipHostMalloc(&h_xstage, sizeof(double) * std::max(n, 1)));
    MMBA_HIP(hipStreamSynchronize(s));
}

// Partitions of the band rows (nested dissection along the frame axis, see
// mmba_band.hip) and the device buffers of the band factorisation.
void Plan::setup_band(int Pforce) {
    const int nb = nR - nG, w = bw;
    // No solved bundle (C2, C5, per-frame solves): the camera-frame blocks are
    // uncoupled, so S is block diagonal + arrow (mmba_bdiag.hip)
    {
        // (nor coupled by the rolling shutter or by a shared lens coefficient)
        if (nB_solved == 0 && nranks == 1 && !cfblk_pc.empty() && Pforce == 0 && !rs_on &&
            !lens_shared) {
            bs.use_bd = true;
            bs.P = 1;
            bs.w = w;
            bs.nb = nb;
            bs.nG = nG;
            bs.Bd = dalloc<double>((size_t)nb * (w + 1));
            bs.Ga = dalloc<double>(std::max<size_t>(1, (size_t)nG * nb));
            bs.Gd = dalloc<double>(NGMAX * NGMAX);
            MMBA_HIP(hipMemsetAsync(bs.Bd, 0, sizeof(double) * (size_t)nb * (w + 1), s));
            MMBA_HIP(hipMemsetAsync(bs.Ga, 0, sizeof(double) * std::max<size_t>(1, (size_t)nG * nb), s));
            MMBA_HIP(hipMemsetAsync(bs.Gd, 0, sizeof(double) * NGMAX * NGMAX, s));
            BdDev &D = bs.bd;
            D.nblk = (int)cfblk_pc.size();
            D.nb = nb;
            D.nG = nG;
            D.w = w;
            int pmax = 1;
            for (int v : cfblk_pc) pmax = std::max(pmax, v);
            D.PC = pmax <= 8 ? 8 : PCMAX;
            D.roff = upload(cfblk_roff);
            D.pc = upload(cfblk_pc);
            D.cf = upload(cfblk_cf);
            D.ticket = dalloc<unsigned int>(1);
            D.part = dalloc<double>((D.nblk + 3) / 4);
            MMBA_HIP(hipMemsetAsync(D.ticket, 0, sizeof(unsigned int), s));
            D.Bd = bs.Bd;
            D.Ga = bs.Ga;
            D.Gd = bs.Gd;
            D.FC = dalloc<double>((size_t)D.nblk * PCMAX * PCMAX);
            D.FY = dalloc<double>((size_t)D.nblk * NGMAX * PCMAX);
            D.Zc = dalloc<double>((size_t)D.nblk * NGMAX * NGMAX);
            D.gpart = dalloc<double>((size_t)D.nblk * NGMAX);
            D.FT = dalloc<double>(NGMAX * NGMAX);
            d_ymask = upload(std::vector<int>(std::max(nR, 1), 1));
            return;
        }
    }
    // w <= 32: the log-depth solvers, block cyclic reduction (mmba_bcr.hip) or
    // parallel cyclic reduction (mmba_pcr.hip).  Pforce < 0 forces them,
    // Pforce > 0 the partitioned chain.
    {
        // Sharded: the partitioned chain's separator system grows with the
        // shard count (one workgroup, (P-1) w rows at bandwidth 2w-1), so the
        // shards all-reduce S instead and each runs the log-depth solve on
        // it; MMBA_PATH_SHARD_BCR = 0 keeps the partitioned chain (tests)
        const bool shard_ok = nranks == 1 || path_choice(MMBA_PATH_SHARD_BCR) != 0;
        // the root (block 0 + the arrow corner) is one wave: K + nG <= 64
        const bool root_fits = std::max(8, (w + 7) / 8 * 8) + (nG + 7) / 8 * 8 <= 64;
        if (shard_ok && w <= 32 && Pforce <= 0 && !sep_form(w) && root_fits) {
            bs.use_bcr = true;
            bs.P = 1;
            bs.comm = nranks > 1 ? comm : nullptr;
            bs.w = w;
            bs.nb = nb;
            bs.nG = nG;
            if (nranks > 1) {
                const size_t nbd = (size_t)nb * (w + 1), nga = (size_t)nG * nb;
                bs.red_count = nbd + nga + NGMAX * NGMAX + (size_t)nRpad;
                bs.red = dalloc<double>(bs.red_count);
                bs.Bd = bs.red;
                bs.Ga = bs.Bd + nbd;
                bs.Gd = bs.Ga + nga;
                bs.red_rhs = bs.Gd + NGMAX * NGMAX;
            } else {
                bs.Bd = dalloc<double>((size_t)nb * (w + 1));
                bs.Ga = dalloc<double>((size_t)nG * nb);
                bs.Gd = dalloc<double>(NGMAX * NGMAX);
            }
            // zeroed once: structural zeros of the band are never written
            MMBA_HIP(hipMemsetAsync(bs.Bd, 0, sizeof(double) * (size_t)nb * (w + 1), s));
            MMBA_HIP(hipMemsetAsync(bs.Ga, 0, sizeof(double) * std::max<size_t>(1, (size_t)nG * nb), s));
            MMBA_HIP(hipMemsetAsync(bs.Gd, 0, sizeof(double) * NGMAX * NGMAX, s));
            BcrDev &B = bs.bcr;
            B.K = std::max(8, (w + 7) / 8 * 8);
            B.nb = nb;
            B.nG = nG;
            B.w = w;
            B.nblk = std::max(1, (nb + B.K - 1) / B.K);
            B.NR = B.K + (nG + 7) / 8 * 8;
            B.Bd = bs.Bd;
            B.Ga = bs.Ga;
            B.Gd = bs.Gd;
            const size_t kk = (size_t)B.nblk * B.K * B.K;
            B.Dk = dalloc<double>(kk);
            B.Lk0 = dalloc<double>(kk);
            B.Lk1 = dalloc<double>(kk);
            B.FC = dalloc<double>(kk);
            B.FU = dalloc<double>(kk);
            B.FV = dalloc<double>(kk);
            B.Gk = dalloc<double>((size_t)B.nblk * nG * B.K);
            B.FY = dalloc<double>((size_t)B.nblk * nG * B.K);
            B.Zc = dalloc<double>((size_t)B.nblk * nG * nG);
            B.FT = dalloc<double>((size_t)B.NR * B.NR);
            B.gpart = dalloc<double>((size_t)B.nblk * nG);
            B.rw = dalloc<double>((size_t)nb + nG);
            {
                if (path_choice(MMBA_PATH_BCR_DATAFLOW) != 0) {
                    B.fflags = dalloc<int>((size_t)B.nblk + 64);  // items < nblk + levels
                    MMBA_HIP(hipMemsetAsync(B.fflags, 0, sizeof(int) * ((size_t)B.nblk + 64), s));
                }
                B.tick = dalloc<unsigned>(2);
                MMBA_HIP(hipMemsetAsync(B.tick, 0, sizeof(unsigned) * 2, s));
                if (path_choice(MMBA_PATH_BCR_GRID) > 0)
                    bs.df_grid = std::max(1, std::min(256, path_choice(MMBA_PATH_BCR_GRID)));
            }
            {
                // dataflow backward solve: blocks in dependency order (root,
                // then levels coarse to fine)
                {
                    std::vector<int> ord{0};
                    int L = 0;
                    while ((1 << L) < B.nblk) ++L;
                    for (int l = L; l >= 0; --l)
                        for (int o = 1 << l; o < B.nblk; o += 2 << l) ord.push_back(o);
                    if ((int)ord.size() != B.nblk) throw Invalid{"bcr order"};
                    B.ord = upload(ord);
                    B.flags = dalloc<int>(B.nblk);
                    MMBA_HIP(hipMemsetAsync(B.flags, 0, sizeof(int) * B.nblk, s));
                }
            }
            // every shard holds the whole y = L^-1 v: rank 0 counts it
            d_ymask = upload(std::vector<int>(std::max(nR, 1), rank == 0 ? 1 : 0));
            // no arrow and K <= 24: parallel cyclic reduction (mmba_pcr.hip)
            // when every block's workgroup fits on the device at once
            {
                // Pforce == -2 (mmba_debug_band_solve): block cyclic reduction only
                const bool pcr_off = path_choice(MMBA_PATH_PCR) == 0 || Pforce == -2;
                // shards take the agreed (smallest) bound: the same solver,
                // hence the same bits, on every shard
                const int kres = std::min(B.K / 8 - 1, 2);
                const int resident = B.K > 24 ? 0
                                     : (nranks > 1 && shard_resident[kres] >= 0)
                                         ? shard_resident[kres]
                                         : pcr_max_resident(B.K);
                if (!pcr_off && nG == 0 && B.K <= 24 && pcr_grid(B.nblk) <= resident) {
                    PcrDev &Q = bs.pcr;
                    Q.K = B.K;
                    // MMBA_PATH_PCR_WIDE = 0 pins the 256-thread form (no pin forces the
                    // 512-thread form: beyond its residency workgroups would wait on
                    // blocks that are not running)
                    Q.nth = path_choice(MMBA_PATH_PCR_WIDE) != 0 &&
                                    pcr_grid(B.nblk) <= pcr_resident_wide(B.K)
                                ? 512
                                : 256;
                    Q.nb = nb;
                    Q.w = w;
                    Q.nblk = B.nblk;
                    int L = 0;
                    while ((1 << L) < B.nblk) ++L;  // block 0 is coupled until 2^L >= nblk
                    Q.nlev = L;
                    Q.Bd = bs.Bd;
                    // publications (levels 0..L-1): P^T [P rho], Q^T [Q rho], Q^T P;
                    // logs (levels 0..L): C^-1, P, Q; right-hand-side pass: 2 K
                    const size_t ps = (size_t)2 * Q.K * (Q.K + 1) + (size_t)Q.K * Q.K;
                    // 16-B granules, one per published double; zeroed (no
                    // stale tag can match: epochs start at 1)
                    Q.pub = dalloc<double>(std::max<size_t>(1, (size_t)2 * L * Q.nblk * ps));
                    MMBA_HIP(hipMemsetAsync(Q.pub, 0, sizeof(double) * std::max<size_t>(1, (size_t)2 * L * Q.nblk * ps), s));
                    Q.wlog = dalloc<double>((size_t)(L + 1) * Q.nblk * 3 * Q.K * Q.K);
                    Q.rpub = dalloc<double>(std::max<size_t>(1, (size_t)L * Q.nblk * 4 * Q.K));  // granules
                    MMBA_HIP(hipMemsetAsync(Q.rpub, 0, sizeof(double) * std::max<size_t>(1, (size_t)L * Q.nblk * 4 * Q.K), s));
                    Q.part = dalloc<double>(Q.nblk);
                    Q.flev = dalloc<int>(Q.nblk);
                    MMBA_HIP(hipMemsetAsync(Q.flev, 0, sizeof(int) * Q.nblk, s));
                    bs.use_pcr = true;
                }
            }
            return;
        }
    }
    if (Ra_all.empty()) {
        Ra_all.assign(1, 0);
        Rb_all.assign(1, nb);
    }
    // partitions per shard range [Ra_all[k], Rb_all[k]) (one range unsharded)
    const bool sepf = sep_form(w);
    // the partitioned chain's windows carry arrows up to NGPART wide; a wider
    // arrow factors the band as one partition (sharded: refused -- block
    // cyclic reduction takes sharded arrows up to 64 - K)
    const bool one_part = !sepf && nG > NGPART;
    if (one_part && Ra_all.size() > 1)
        throw Unsupported{"more than " + std::to_string(NGPART) +
                          " global parameters on a sharded band plan"};
    auto count_parts = [&](int len) {
        int P = 1;
        if (one_part) {
        } else if (sepf) {
            // separator form: the shard's range is one partition
        } else if (Pforce > 0 && w <= WBAND_PART) {
            P = std::max(1, std::min(Pforce, len / (w + 1)));
        } else if (w > 0 && w <= WBAND_PART) {
            // balance the interior chains (len/P rows) against the separator
            // chain ((P-1) w rows at bandwidth 2w-1); measured on C4 (nb 2994,
            // w 23): P = 1/4/8/12/16/24 -> 1.20/0.70/0.44/0.40/0.41/0.48 ms
            P = (int)std::lround(std::sqrt((double)len / w));
            P = std::max(1, std::min(P, len / (2 * w + 8)));
        }
        return P;
    };
    std::vector<std::pair<int, int>> spans;  // [s0, s1) of every partition
    for (size_t k = 0; k < Ra_all.size(); ++k) {
        const int a = Ra_all[k], len = Rb_all[k] - a;
        const int Pk = count_parts(len);
        if ((int)k == rank) bs.p_lo = (int)spans.size();
        for (int p = 0; p < Pk; ++p)
            spans.push_back({a + (int)((long long)p * len / Pk),
                             a + (int)((long long)(p + 1) * len / Pk)});
        if ((int)k == rank) bs.p_hi = (int)spans.size();
    }
    const int P = (int)spans.size();
    std::vector<BandPart> parts(P);
    long long aoff = 0;
    int zoff = 0, doff = 0, coff = 0;
    bs.max_arrow = 0;
    for (int p = 0; p < P; ++p) {
        BandPart &q = parts[p];
        const int s0 = spans[p].first, s1 = spans[p].second;
        q.r0 = s0;
        q.r1 = (p < P - 1) ? s1 - w : s1;
        q.nprev = p > 0 ? w : 0;
        q.nnext = p < P - 1 ? w : 0;
        q.sprev = p > 0 ? s0 - w : -1;
        q.snext = p < P - 1 ? s1 - w : -1;
        q.na = q.nprev + q.nnext + nG;
        q.aoff = P > 1 ? aoff : 0;
        q.zoff = zoff;
        q.doff = doff;
        q.coff = coff;
        aoff += (long long)q.na * (q.r1 - q.r0);
        bs.max_arrow = std::max(bs.max_arrow, (long long)q.na * (q.r1 - q.r0));
        zoff += q.na * (q.na + 1) / 2;
        doff += (q.r1 - q.r0 + 7) / 8;
        coff += q.na;
    }
    // ||L^-1 v||^2 terms counted by this shard: its interior rows; the
    // separator and global rows (replicated) on the root shard.  Separator
    // form: the interior's share is v^T S_II^-1 v = v . y (mask 2)
    {
        std::vector<int> ym(nR, 0);
        for (int p = bs.p_lo; p < bs.p_hi; ++p)
            for (int r = parts[p].r0; r < parts[p].r1; ++r) ym[r] = sepf ? 2 : 1;
        if (rank == 0) {
            for (int p = 0; p < P - 1; ++p)
                for (int u = 0; u < w; ++u) ym[parts[p].snext + u] = 1;
            for (int q = nb; q < nR; ++q) ym[q] = 1;
        }
        d_ymask = upload(ym);
    }
    bs.P = P;
    bs.comm = nranks > 1 ? comm : nullptr;
    bs.w = w;
    bs.nb = nb;
    bs.nG = nG;
    bs.Bd = dalloc<double>((size_t)nb * (w + 1));
    bs.Ga = dalloc<double>((size_t)nG * nb);
    bs.Gd = dalloc<double>(NGMAX * NGMAX);
    bs.Gdinv = dalloc<double>(NGMAX * NGMAX);
    bs.Dinv = dalloc<double>((size_t)doff * 64);
    bs.d_parts = upload(parts);
    if (P > 1) {
        bs.apool = dalloc<double>((size_t)aoff);
        bs.zpool = dalloc<double>((size_t)zoff);
        bs.cpool = dalloc<double>((size_t)coff);
        const int nbT = (P - 1) * w;
        bs.tcount = (size_t)nbT * 2 * w + (size_t)nG * nbT + NGMAX * NGMAX;
        bs.TBd = dalloc<double>(bs.tcount);
        bs.TGa = bs.TBd + (size_t)nbT * 2 * w;
        bs.TGd = bs.TGa + (size_t)nG * nbT;
        bs.TGdinv = dalloc<double>(NGMAX * NGMAX);
        bs.TDinv = dalloc<double>((size_t)((nbT + 7) / 8) * 64);
        BandPart t{};
        t.r0 = 0;
        t.r1 = nbT;
        t.na = nG;
        t.sprev = t.snext = -1;
        bs.d_tpart = upload(std::vector<BandPart>{t});
        bs.rT = dalloc<double>(nbT + nG);
        bs.yT = dalloc<double>(nbT + nG);
        bs.xT = dalloc<double>(nbT + nG);
    }
    if (sepf) {
        // the shard's interior by parallel cyclic reduction (mmba_pcr.hip) on
        // its rows of Bd: the band layout is row-relative, so an offset view
        // is the interior system with its couplings to the separators dropped
        const BandPart &hp = parts[bs.p_lo];
        const int ast = hp.r1 - hp.r0;
        bs.pcr_int = true;
        bs.hpart = hp;
        bs.fail = d_fail;
        PcrDev &Q = bs.ipcr;
        Q.K = std::max(8, (w + 7) / 8 * 8);
        // (one process's PCR launches on a device are ordered, pcr_ordered)
        Q.nth = path_choice(MMBA_PATH_PCR_WIDE) != 0 &&
                        pcr_grid((hp.r1 - hp.r0 + Q.K - 1) / Q.K) <= pcr_resident_wide(Q.K)
                    ? 512
                    : 256;
        Q.nb = ast;
        Q.w = w;
        Q.nblk = (ast + Q.K - 1) / Q.K;
        int L = 0;
        while ((1 << L) < Q.nblk) ++L;
        Q.nlev = L;
        Q.Bd = bs.Bd + (size_t)hp.r0 * (w + 1);
        const size_t ps = (size_t)2 * Q.K * (Q.K + 1) + (size_t)Q.K * Q.K;
        const size_t nl = std::max<size_t>(1, (size_t)L * Q.nblk);
        Q.pub = dalloc<double>(2 * nl * ps);  // 16-B granules (k_pcr_solve), zeroed
        MMBA_HIP(hipMemsetAsync(Q.pub, 0, sizeof(double) * 2 * nl * ps, s));
        Q.wlog = dalloc<double>((size_t)(L + 1) * Q.nblk * 3 * Q.K * Q.K);
        Q.rpub = dalloc<double>(nl * 4 * Q.K);  // granules (k_pcr_rhs), zeroed
        MMBA_HIP(hipMemsetAsync(Q.rpub, 0, sizeof(double) * nl * 4 * Q.K, s));
        Q.mpub = dalloc<double>(nl * 4 * Q.K * PCR_NCMAX);  // granules (k_pcr_rhs_mc), zeroed
        MMBA_HIP(hipMemsetAsync(Q.mpub, 0, sizeof(double) * nl * 4 * Q.K * PCR_NCMAX, s));
        Q.part = dalloc<double>(Q.nblk);
        Q.flev = dalloc<int>(Q.nblk);
                    MMBA_HIP(hipMemsetAsync(Q.flev, 0, sizeof(int) * Q.nblk, s));
        bs.XA = dalloc<double>((size_t)std::max(hp.na, 1) * ast);
        bs.izero = dalloc<double>(ast);
        bs.ix = dalloc<double>(ast);
        MMBA_HIP(hipMemsetAsync(bs.izero, 0, sizeof(double) * ast, s));
    }
}

// Separator form of the sharded reduced solve: every
// shard eliminates the interior of its row range by parallel cyclic
// reduction, only the separator system (the last w rows of every shard but
// the last, with the shards' Schur terms) is all-reduced and solved on every
// shard.  Needs no arrow, w <= 23 and every shard's interior resident on the
// device; every shard decides the same from the shared partition and the
// smallest residency bound of the shards' devices (all-reduced by
// mmba_plan_create_sharded before any shard builds, so that no build-time
// failure can leave a shard in another collective than its peers: a shard on
// a device with fewer CUs must not take another path than the rest, whose
// collectives would then differ).  No collective here.
bool Plan::sep_form(int w) {
    if (nranks <= 1 || nG != 0 || w > 23 || w <= 0) return false;
    // Default (round 5): the whole-S form while the WHOLE band system fits one
    // resident PCR grid (C4 shards: N <= 4), the separator form beyond -- the
    // whole system then falls back to block cyclic reduction (142 us at
    // 998 blocks against PCR's 62 us on one shard's interior; profiles/r5_occ,
    // r5_gran).  The one-device rehearsal of 2/4/8 shards measured the
    // separator form slower (profiles/r5_sep), but there the shards' PCR
    // launches queue behind each other on the one device.  Pinned either way
    // by MMBA_PATH_SHARD_SEP (0 / 1).
    const int pin = path_choice(MMBA_PATH_SHARD_SEP);
    if (pin == 0 || path_choice(MMBA_PATH_SHARD_BCR) == 0) return false;
    const int K = std::max(8, (w + 7) / 8 * 8);
    int most = 0;
    for (size_t k = 0; k < Ra_all.size(); ++k) {
        const int len = Rb_all[k] - Ra_all[k] - ((int)k + 1 < (int)Ra_all.size() ? w : 0);
        if (len < K) return false;
        most = std::max(most, (len + K - 1) / K);
    }
    const int sep_resident = shard_resident[K / 8 - 1];
    if (sep_resident < 0) return false;
    if (pcr_grid(most) > sep_resident) return false;
    if (pin == 1) return true;
    return pcr_grid((nR + K - 1) / K) > sep_resident;  // the whole system would not be resident
}

}  // namespace mmba
