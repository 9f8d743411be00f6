// mmba_metrics.hip -- per-frame and per-marker deviation metrics
// (mmba_plan_error_metrics): what ErrorMetricsResult::fill
// (adjust_results.h:392-463) and create_deviation_attrs_on_node
// (adjust_results_helpers.cpp:213-246) compute from errorDistanceList, reduced
// on the device so that a solve with device-resident outputs hands back
// (num_frames + num_markers) entries instead of the per-residual lists.
//
// One launch reduces every segment (a frame's or a marker's observations):
// count, sum, max (from 0, with >, so a NaN never wins) and the key of the
// max.  A group of W lanes takes a segment: lane l sums entries l, l + W, ...
// in that order, then a fixed xor tree over the W lanes.  W is a function of
// the segment's length alone (metrics_width: markers are short, 4 entries on
// C4, frames long, ~1,650 on C2) and the entries are listed in ascending
// reference order, so a segment's bits depend on nothing but its values in
// that order and their number -- not on the device's observation order, the
// solver path or the shard count.  No atomics; each result is one plain
// store by the group's first lane.
#include <climits>
#include <cstring>

#include "mmba_kernels.h"
#include "mmba_plan.h"

namespace mmba {

template <int W>
__device__ __forceinline__ void metrics_group(const MetricsDev &T, const double *__restrict__ ed,
                                              int q, int end, int lane) {
    const int sub = lane & (W - 1);
    const bool live = q < end;
    const int g = live ? T.seg_list[q] : 0;
    const int a = live ? T.seg_off[g] : 0;
    const int n = live ? T.seg_off[g + 1] - a : 0;
    double sum = 0., mx = 0.;
    int pos = INT_MAX;  // position in the segment of the first entry that set mx
#pragma unroll 4
    for (int p = sub; p < n; p += W) {
        const double v = ed[T.idx[a + p]];
        sum += v;
        if (v > mx) {
            mx = v;
            pos = p;
        }
    }
    // every lane of the wave takes part (dead groups carry zeros); not
    // wave_sum: W lanes, ascending, with the arg-max folded in
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
        const double s2 = __shfl_xor(sum, d), m2 = __shfl_xor(mx, d);
        const int p2 = __shfl_xor(pos, d);
        sum += s2;
        if (m2 > mx || (m2 == mx && p2 < pos)) {
            mx = m2;
            pos = p2;
        }
    }
    if (live && sub == 0) {
        T.res_d[g] = sum;
        T.res_d[T.S + g] = mx;
        T.res_i[g] = n;
        T.res_i[T.S + g] = pos < n ? T.key[a + pos] : -1;
    }
}

__global__ void __launch_bounds__(256) k_error_metrics(MetricsDev T,
                                                       const double *__restrict__ ed) {
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int w4 = (T.n4 + 15) / 16, w16 = (T.n16 + 3) / 4;
    if (gw < w4)
        metrics_group<4>(T, ed, gw * 16 + (lane >> 2), T.n4, lane);
    else if (gw < w4 + w16)
        metrics_group<16>(T, ed, T.n4 + (gw - w4) * 4 + (lane >> 4), T.n4 + T.n16, lane);
    else if (gw < w4 + w16 + T.n64)
        metrics_group<64>(T, ed, T.n4 + T.n16 + (gw - w4 - w16), T.S, lane);
}

// Sharded plans.  coll = [sum | count | max | arg key] (S doubles each): the
// first two are summed over the shards, the third takes their max; a shard
// whose own max is the merged one then offers minus its key, anything else a
// value below every key, and the max of those is minus the lowest key.
static constexpr double kNoKey = -4294967296.0;

__global__ void k_metrics_pack(MetricsDev T, double *__restrict__ coll) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.S) return;
    coll[i] = T.res_d[i];
    coll[T.S + i] = (double)T.res_i[i];
    coll[2 * (size_t)T.S + i] = T.res_d[T.S + i];
}

__global__ void k_metrics_argkey(MetricsDev T, double *__restrict__ coll) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.S) return;
    const int arg = T.res_i[T.S + i];
    coll[3 * (size_t)T.S + i] =
        (arg >= 0 && T.res_d[T.S + i] == coll[2 * (size_t)T.S + i]) ? -(double)arg : kNoKey;
}

__global__ void k_metrics_unpack(MetricsDev T, const double *__restrict__ coll) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.S) return;
    T.res_d[i] = coll[i];
    T.res_i[i] = (int)coll[T.S + i];
    T.res_d[T.S + i] = coll[2 * (size_t)T.S + i];
    const double k = coll[3 * (size_t)T.S + i];
    T.res_i[T.S + i] = k <= kNoKey ? -1 : (int)(-k);
}

void launch_error_metrics(hipStream_t s, const MetricsDev &T, const double *ed) {
    const int waves = (T.n4 + 15) / 16 + (T.n16 + 3) / 4 + T.n64;
    if (waves > 0) k_error_metrics<<<(waves + 3) / 4, 256, 0, s>>>(T, ed);
}
void launch_metrics_pack(hipStream_t s, const MetricsDev &T, double *coll) {
    k_metrics_pack<<<(T.S + 255) / 256, 256, 0, s>>>(T, coll);
}
void launch_metrics_argkey(hipStream_t s, const MetricsDev &T, double *coll) {
    k_metrics_argkey<<<(T.S + 255) / 256, 256, 0, s>>>(T, coll);
}
void launch_metrics_unpack(hipStream_t s, const MetricsDev &T, const double *coll) {
    k_metrics_unpack<<<(T.S + 255) / 256, 256, 0, s>>>(T, coll);
}

// The segment table (F frames, then K markers), one index list and one key
// list per axis over this shard's own observations in ascending reference
// order (a counting sort by segment), and the segments by lane-group width.
// From the global problem: every shard lists the same segments.
void Plan::setup_metrics(int F_, int K, int Mg_, const int32_t *obs_marker,
                         const int32_t *obs_frame, const std::vector<int> &dev_of_own) {
    met_F = F_;
    met_K = K;
    const int S = F_ + K;
    std::vector<int> seg_off(S + 1, 0);
    for (int r = 0; r < Mg_; ++r) {
        if (dev_of_own[r] < 0) continue;
        seg_off[obs_frame[r] + 1]++;
        seg_off[F_ + obs_marker[r] + 1]++;
    }
    for (int g = 0; g < S; ++g) seg_off[g + 1] += seg_off[g];
    const int total = seg_off[S];
    std::vector<int> idx(std::max(total, 1), 0), key(std::max(total, 1), 0);
    std::vector<int> fill(seg_off.begin(), seg_off.end() - 1);
    for (int r = 0; r < Mg_; ++r) {
        const int d = dev_of_own[r];
        if (d < 0) continue;
        const int qf = fill[obs_frame[r]]++, qm = fill[F_ + obs_marker[r]]++;
        idx[qf] = d;
        key[qf] = obs_marker[r];
        idx[qm] = d;
        key[qm] = obs_frame[r];
    }
    std::vector<int> seg_list(std::max(S, 1), 0);
    int cnt[3] = {0, 0, 0};
    auto cls = [&](int g) {
        const int w = metrics_width(seg_off[g + 1] - seg_off[g]);
        return w == 4 ? 0 : w == 16 ? 1 : 2;
    };
    for (int g = 0; g < S; ++g) cnt[cls(g)]++;
    int at[3] = {0, cnt[0], cnt[0] + cnt[1]};
    for (int g = 0; g < S; ++g) seg_list[at[cls(g)]++] = g;
    met.S = S;
    met.n4 = cnt[0];
    met.n16 = cnt[1];
    met.n64 = cnt[2];
    met.seg_off = upload(seg_off);
    met.idx = upload(idx);
    met.key = upload(key);
    met.seg_list = upload(seg_list);
    // [sum | max] doubles then [count | arg] ints, one block: one copy per call
    char *blk = dalloc<char>(24 * (size_t)std::max(S, 1));
    met.res_d = reinterpret_cast<double *>(blk);
    met.res_i = reinterpret_cast<int *>(blk + 16 * (size_t)S);
    MMBA_HIP(hipHostMalloc((void **)&h_met, 24 * (size_t)std::max(S, 1), hipHostMallocDefault));
    if (nranks > 1) d_met_coll = dalloc<double>(4 * (size_t)std::max(S, 1));
}

void Plan::error_metrics(mmba_error_metrics *out) {
    const int S = met.S;
    launch_error_metrics(s, met, d_ed);
    if (nranks > 1) {
        launch_metrics_pack(s, met, d_met_coll);
        allreduce(d_met_coll, 2 * (size_t)S);
        allreduce(d_met_coll + 2 * (size_t)S, S, ReduceOp::Max);
        launch_metrics_argkey(s, met, d_met_coll);
        allreduce(d_met_coll + 3 * (size_t)S, S, ReduceOp::Max);
        launch_metrics_unpack(s, met, d_met_coll);
    }
    MMBA_HIP(hipMemcpyAsync(h_met, met.res_d, 24 * (size_t)S, hipMemcpyDeviceToHost, s));
    stream_wait();
    if (!out) return;
    const double *sum = reinterpret_cast<const double *>(h_met), *mx = sum + S;
    const int *cnt = reinterpret_cast<const int *>(h_met + 16 * (size_t)S), *arg = cnt + S;
    auto avg = [&](int g) { return cnt[g] > 0 ? sum[g] / (double)cnt[g] : 0.; };
    const int F_ = met_F, K = met_K;
    if (out->frame_count) std::memcpy(out->frame_count, cnt, sizeof(int) * F_);
    if (out->frame_max) std::memcpy(out->frame_max, mx, sizeof(double) * F_);
    if (out->frame_max_marker) std::memcpy(out->frame_max_marker, arg, sizeof(int) * F_);
    if (out->frame_avg)
        for (int f = 0; f < F_; ++f) out->frame_avg[f] = avg(f);
    if (out->marker_count) std::memcpy(out->marker_count, cnt + F_, sizeof(int) * K);
    if (out->marker_max) std::memcpy(out->marker_max, mx + F_, sizeof(double) * K);
    if (out->marker_max_frame) std::memcpy(out->marker_max_frame, arg + F_, sizeof(int) * K);
    if (out->marker_avg)
        for (int k = 0; k < K; ++k) out->marker_avg[k] = avg(F_ + k);
}

}  // namespace mmba
