// mmba_lens_shared.hip -- an animated lens coefficient read by several
// cameras' rows at its frame (C5 with focus breathing: two cameras, one
// lens).
//
// Plan::build puts such a coefficient into the block of one host
// camera-frame of its frame (a VF_LENS variant, as the one-camera form) and
// lists the other camera-frames of the frame whose rows read it: the foreign
// readers.  A foreign row carries the coefficient's column after its bundle
// columns, with the parameter id in jcol (k_jacobian's lens loop).  The
// camera-frame pass (k_ne_cf and its uniform forms) sums each block over its
// own rows only, so what the foreign rows add is formed here, per host:
//   Acc(host)[h, h'] += sum J_h J_h'      g[h] += sum J_h f
//   Acg(host)[h, q]  += sum J_h J_q       (q: the remaining global parameters)
// and per link (foreign camera-frame X, host) the coupling block
//   A(X, host)[a, h] = sum J_a J_h        (a: X's own block columns),
// which k_lens_shared_offdiag writes into the reduced system after
// k_schur_init, as k_rs_offdiag does for the rolling shutter.  The host's own
// pose columns never appear in a foreign row: those products are structurally
// zero and not formed.  One thread per output entry, the observations in a
// fixed order, one store per entry: bit-identical from call to call.
#include <hip/hip_runtime.h>

#include "mmba_kernels.h"

namespace mmba {

constexpr int LS_CHUNK = 64;
// a host task's entries: nh (nh + 1) / 2 + nh + nh nG <= 78 + 12 + 576
constexpr int LS_EPT = (PCMAX * (PCMAX + 1) / 2 + PCMAX + PCMAX * NGMAX + 255) / 256;

struct LsTab {
    const int *host, *nh, *link_off, *hpar, *hpos, *link_cf, *link_grp;
};
__device__ __forceinline__ LsTab ls_tab(const DevProblem &P) {
    LsTab T;
    T.host = P.ls_tab;
    T.nh = T.host + P.ls_ng;
    T.link_off = T.nh + P.ls_ng;
    T.hpar = T.link_off + P.ls_ng + 1;
    T.hpos = T.hpar + (size_t)P.ls_ng * PCMAX;
    T.link_cf = T.hpos + (size_t)P.ls_ng * PCMAX;
    T.link_grp = T.link_cf + P.ls_nl;
    return T;
}

// Workgroups [0, ls_ng): a host's additions over the rows of all its links,
// in link order.  Workgroups ls_ng + k: the coupling block of link k.
__global__ void __launch_bounds__(256) k_ne_lens_shared(DevProblem P, const double *__restrict__ J,
                                                        const int *__restrict__ jcol,
                                                        const int *__restrict__ nloc,
                                                        const double *__restrict__ f, double *Acc,
                                                        double *Acg, double *g, double *Aoff) {
    __shared__ double sJ[2 * LMAX][LS_CHUNK];
    __shared__ int sG[NGMAX][LS_CHUNK];  // local column of global q in observation o (-1)
    __shared__ int sH[PCMAX][LS_CHUNK];  // local column of hosted coefficient h (-1)
    __shared__ double sF[2][LS_CHUNK];
    const LsTab T = ls_tab(P);
    const bool coup = (int)blockIdx.x >= P.ls_ng;
    const int link = coup ? blockIdx.x - P.ls_ng : -1;
    const int grp = coup ? T.link_grp[link] : blockIdx.x;
    const int H = T.host[grp], nh = T.nh[grp];
    const int k0 = coup ? link : T.link_off[grp], k1 = coup ? link + 1 : T.link_off[grp + 1];
    const int *hpar = &T.hpar[(size_t)grp * PCMAX], *hpos = &T.hpos[(size_t)grp * PCMAX];
    const int nG = coup ? 0 : P.nG;  // a coupling block needs no global columns
    const int nCF = P.nR - P.nG;
    const int lm = P.lmax;
    const size_t M = P.M;
    const int nhh = nh * (nh + 1) / 2;
    const int nent = coup ? P.cf_pc[T.link_cf[link]] * nh : nhh + nh + nh * nG;
    // kind 0: hosted x hosted, 1: hosted x f, 2: hosted x global, 3: coupling
    int kind[LS_EPT], ea[LS_EPT], eb[LS_EPT];
    double acc[LS_EPT];
#pragma unroll
    for (int j = 0; j < LS_EPT; ++j) {
        const int e = threadIdx.x + 256 * j;
        kind[j] = -1;
        ea[j] = eb[j] = 0;
        acc[j] = 0.;
        if (e >= nent) continue;
        if (coup) {
            kind[j] = 3;
            ea[j] = e / nh;
            eb[j] = e % nh;
        } else if (e < nhh) {
            int rem = e, r = 0;
            while (rem >= nh - r) {
                rem -= nh - r;
                ++r;
            }
            kind[j] = 0;
            ea[j] = r;
            eb[j] = r + rem;
        } else if (e < nhh + nh) {
            kind[j] = 1;
            ea[j] = e - nhh;
        } else {
            kind[j] = 2;
            ea[j] = (e - nhh - nh) / nG;
            eb[j] = (e - nhh - nh) % nG;
        }
    }
    for (int k = k0; k < k1; ++k) {
        const int X = T.link_cf[k];
        const int o0 = P.cf_obs_off[X], o1 = P.cf_obs_off[X + 1];
        for (int c0 = o0; c0 < o1; c0 += LS_CHUNK) {
            const int cnt = min(LS_CHUNK, o1 - c0);
            __syncthreads();
            for (int t = threadIdx.x; t < 2 * lm * LS_CHUNK; t += blockDim.x) {
                const int row = t / LS_CHUNK, o = t % LS_CHUNK;
                sJ[row][o] = (o < cnt) ? J[(size_t)row * M + c0 + o] : 0.;
            }
            for (int t = threadIdx.x; t < PCMAX * LS_CHUNK; t += blockDim.x)
                sH[t / LS_CHUNK][t % LS_CHUNK] = -1;
            for (int t = threadIdx.x; t < nG * LS_CHUNK; t += blockDim.x)
                sG[t / LS_CHUNK][t % LS_CHUNK] = -1;
            __syncthreads();
            for (int t = threadIdx.x; t < lm * LS_CHUNK; t += blockDim.x) {
                const int l = t / LS_CHUNK, o = t % LS_CHUNK;
                if (o >= cnt || l >= nloc[c0 + o]) continue;
                const int p = jcol[(size_t)l * M + c0 + o];
                const int cls = P.p_class[p];
                if (cls == PC_CF && P.p_blk[p] == H) {
                    for (int h = 0; h < nh; ++h)
                        if (hpar[h] == p) sH[h][o] = l;
                } else if (cls == PC_G && nG > 0) {
                    sG[P.p_pos[p] - nCF][o] = l;
                }
            }
            if (!coup)
                for (int t = threadIdx.x; t < LS_CHUNK; t += blockDim.x) {
                    sF[0][t] = (t < cnt) ? f[2 * (size_t)(c0 + t)] : 0.;
                    sF[1][t] = (t < cnt) ? f[2 * (size_t)(c0 + t) + 1] : 0.;
                }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < LS_EPT; ++j) {
                if (kind[j] < 0) continue;
                double a = acc[j];
                if (kind[j] == 3) {
                    const int la = ea[j];  // X's own block columns come first
                    for (int o = 0; o < cnt; ++o) {
                        const int lb = sH[eb[j]][o];
                        if (lb >= 0)
                            a += sJ[2 * la][o] * sJ[2 * lb][o] + sJ[2 * la + 1][o] * sJ[2 * lb + 1][o];
                    }
                } else if (kind[j] == 0) {
                    for (int o = 0; o < cnt; ++o) {
                        const int la = sH[ea[j]][o], lb = sH[eb[j]][o];
                        if (la >= 0 && lb >= 0)
                            a += sJ[2 * la][o] * sJ[2 * lb][o] + sJ[2 * la + 1][o] * sJ[2 * lb + 1][o];
                    }
                } else if (kind[j] == 1) {
                    for (int o = 0; o < cnt; ++o) {
                        const int la = sH[ea[j]][o];
                        if (la >= 0) a += sJ[2 * la][o] * sF[0][o] + sJ[2 * la + 1][o] * sF[1][o];
                    }
                } else {
                    for (int o = 0; o < cnt; ++o) {
                        const int la = sH[ea[j]][o], lb = sG[eb[j]][o];
                        if (la >= 0 && lb >= 0)
                            a += sJ[2 * la][o] * sJ[2 * lb][o] + sJ[2 * la + 1][o] * sJ[2 * lb + 1][o];
                    }
                }
                acc[j] = a;
            }
        }
    }
    // the host's entries were stored by the camera-frame pass of this launch_ne
    double *A = &Acc[(size_t)H * PCMAX * PCMAX];
#pragma unroll
    for (int j = 0; j < LS_EPT; ++j) {
        if (kind[j] == 3) {
            Aoff[((size_t)link * PCMAX + ea[j]) * PCMAX + eb[j]] = acc[j];
        } else if (kind[j] == 0) {
            const int ra = hpos[ea[j]], rb = hpos[eb[j]];
            const double v = A[ra * PCMAX + rb] + acc[j];
            A[ra * PCMAX + rb] = v;
            if (ra != rb) A[rb * PCMAX + ra] = v;
        } else if (kind[j] == 1) {
            g[hpar[ea[j]]] += acc[j];
        } else if (kind[j] == 2) {
            Acg[((size_t)H * PCMAX + hpos[ea[j]]) * NGMAX + eb[j]] += acc[j];
        }
    }
}

// The coupling blocks into the reduced system (after k_schur_init):
// S(roff(X) + a, roff(host) + hpos(h)) = A(X, host)_ah.  X is numbered after
// its host (camera-frames are frame-major, the host the frame's first
// reader), so the entry is in the lower triangle and, by Plan::build's bw,
// inside the band.
__global__ void __launch_bounds__(256) k_lens_shared_offdiag(DevProblem P,
                                                             const double *__restrict__ Aoff,
                                                             const SView V) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int link = t / (PCMAX * PCMAX);
    if (link >= P.ls_nl) return;
    const LsTab T = ls_tab(P);
    const int a = (t / PCMAX) % PCMAX, h = t % PCMAX;
    const int X = T.link_cf[link], grp = T.link_grp[link];
    if (a >= P.cf_pc[X] || h >= T.nh[grp]) return;
    *s_at(V, P.cf_roff[X] + a, P.cf_roff[T.host[grp]] + T.hpos[(size_t)grp * PCMAX + h]) =
        Aoff[((size_t)link * PCMAX + a) * PCMAX + h];
}

void launch_ne_lens_shared(hipStream_t s, const DevProblem &P, const double *J, const int *jcol,
                           const int *nloc, const double *f, double *Acc, double *Acg, double *g) {
    if (P.ls_ng + P.ls_nl > 0)
        k_ne_lens_shared<<<P.ls_ng + P.ls_nl, 256, 0, s>>>(P, J, jcol, nloc, f, Acc, Acg, g,
                                                          P.ls_Aoff);
}

void launch_lens_shared_offdiag(hipStream_t s, const DevProblem &P, const SView &V) {
    const long n = (long)P.ls_nl * PCMAX * PCMAX;
    if (n > 0) k_lens_shared_offdiag<<<(int)((n + 255) / 256), 256, 0, s>>>(P, P.ls_Aoff, V);
}

}  // namespace mmba
