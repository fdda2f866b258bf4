// ss_em_strain_sets: read-based strain abundances by EM over the equivalence classes of ss_reads_classify_strains
// (`--em_strains`), many count vectors -- the sample's and its bootstrap replicates' -- in one launch.
//
// The rule is in strainscan_hip.h and, in numpy, in tests/em_model.py.  One iteration is, per set with reads, d = the rho of its
// strains added up and q = n / d, and per strain the sum of the q of the sets that hold it; rho'_j = rho_j * that sum / N.
//
// em_kernel, one workgroup of 256 threads per vector, float64 throughout:
//   * STAGED (n_sets <= SS_EM_LDS_SETS): the masks (2 bytes) and the counts as doubles (8 bytes) of the vector are put in LDS once
//     -- 60 KB at 6144 sets, which leaves room for two workgroups on a CU -- else every iteration reads them from global memory.
//   * rho[16] and the sixteen partial sums are registers of every thread (64 VGPRs; all indices are compile-time, nothing is
//     indexed dynamically).  A thread walks the sets t, t + 256, ...: sixteen selects and adds for d, ONE division, sixteen selects
//     and adds for the sums.  There is no multiplication next to an addition, so nothing contracts to an FMA and every step rounds
//     as the model's does.
//   * The sums meet in a FIXED order: within the wave a halving exchange -- lanes l and l ^ 32 split the sixteen sums between
//     them (eight 64-bit shuffles, not sixteen), l ^ 16 the eight that are left, then 4, 2, 1, and two plain steps over l ^ 2 and
//     l ^ 1: 17 shuffles of a double for all sixteen sums, after which lane 4 j holds sum j of the wave -- then the four waves
//     through LDS, added in wave order by thread j.  No floating-point atomics: the same input gives the same bits.
//   * Threads 0..15 finish their strain and leave rho' and |rho' - rho| in LDS; every thread reads all sixteen back and takes the
//     largest difference itself, so the workgroup agrees on stopping without a third barrier.  One launch per call.
// N and the active strains are taken in integers (a wave reduction, then LDS atomics on integers: exact in any order).
#include "ss_common.h"
#include "ss_support.h"

#include <vector>

namespace {

constexpr uint32_t EM_THREADS = 256, EM_WAVES = EM_THREADS / 64, EM_L = SS_STRAIN_SET_MAX;
static_assert(EM_L == 16, "the wave reduction halves sixteen sums four times");
static_assert(SS_EM_LDS_SETS * 10u + EM_WAVES * EM_L * 8u + 2u * EM_L * 8u + 64u <= 64u * 1024u, "the staged vector fits 64 KB of LDS");

__device__ __forceinline__ double shfl_xor_f64(double x, int m)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __shfl_xor(lo, m, 64);
    hi = __shfl_xor(hi, m, 64);
    return __hiloint2double(hi, lo);
}

// a[0..2H) of every lane -> a[0..H): the lanes with bit `bit` clear keep the lower half, the others the upper, each plus its
// partner's part of the same sums
template <int H>
__device__ __forceinline__ void halve(double (&a)[EM_L], uint32_t lane, int bit)
{
    const bool up = (lane & (uint32_t)bit) != 0u;
#pragma unroll
    for (int i = 0; i < H; i++) {
        const double send = up ? a[i] : a[i + H], keep = up ? a[i + H] : a[i];
        a[i] = keep + shfl_xor_f64(send, bit);
    }
}

template <bool STAGED>
__global__ __launch_bounds__(EM_THREADS) void em_kernel(const unsigned long long *__restrict__ counts, const uint16_t *__restrict__ masks,
                                                        uint32_t n_sets, uint32_t n_strains, uint32_t max_iter, double tol,
                                                        double *__restrict__ rho_out, uint32_t *__restrict__ iters_out)
{
    __shared__ double s_n[STAGED ? SS_EM_LDS_SETS : 1];
    __shared__ uint16_t s_mask[STAGED ? SS_EM_LDS_SETS : 1];
    __shared__ double s_part[EM_WAVES][EM_L];
    __shared__ double s_rho[EM_L], s_delta[EM_L];
    __shared__ unsigned long long s_total;
    __shared__ uint32_t s_active;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned long long *cv = counts + (size_t)blockIdx.x * n_sets;
    if (t == 0) { s_total = 0ull; s_active = 0u; }
    __syncthreads();
    // N, the active strains and the staged copy
    unsigned long long tot = 0;
    uint32_t act = 0;
    for (uint32_t s = t; s < n_sets; s += EM_THREADS) {
        const unsigned long long c = cv[s];
        const uint32_t m = masks[s];
        if (STAGED) { s_n[s] = (double)c; s_mask[s] = (uint16_t)m; }
        tot += c;
        if (c) act |= m;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        tot += ((unsigned long long)(uint32_t)__shfl_xor((int)(tot >> 32), m, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)tot, m, 64);
        act |= (uint32_t)__shfl_xor((int)act, m, 64);
    }
    if (lane == 0) { atomicAdd(&s_total, tot); atomicOr(&s_active, act); }
    __syncthreads();
    const unsigned long long total = s_total;
    const uint32_t active = s_active;
    double *out = rho_out + (size_t)blockIdx.x * n_strains;
    if (total == 0ull) {                                            // (uniform)
        if (t < n_strains) out[t] = 0.0;
        if (t == 0) iters_out[blockIdx.x] = 0u;
        return;
    }
    const double N = (double)total, start = 1.0 / (double)__popc(active);
    double rho[EM_L];
#pragma unroll
    for (uint32_t j = 0; j < EM_L; j++) rho[j] = (active >> j) & 1u ? start : 0.0;
    uint32_t it = 0;
    for (;;) {
        double acc[EM_L];
#pragma unroll
        for (uint32_t j = 0; j < EM_L; j++) acc[j] = 0.0;
        for (uint32_t s = t; s < n_sets; s += EM_THREADS) {
            const double n = STAGED ? s_n[s] : (double)cv[s];
            const uint32_t m = STAGED ? s_mask[s] : masks[s];
            double d = 0.0;
#pragma unroll
            for (uint32_t j = 0; j < EM_L; j++) d += (m >> j) & 1u ? rho[j] : 0.0;
            if (n > 0.0 && d > 0.0) {
                const double q = n / d;
#pragma unroll
                for (uint32_t j = 0; j < EM_L; j++) acc[j] += (m >> j) & 1u ? q : 0.0;
            }
        }
        halve<8>(acc, lane, 32);
        halve<4>(acc, lane, 16);
        halve<2>(acc, lane, 8);
        halve<1>(acc, lane, 4);
        acc[0] += shfl_xor_f64(acc[0], 2);
        acc[0] += shfl_xor_f64(acc[0], 1);
        // lane l holds sum ((l >> 5) & 1) * 8 + ((l >> 4) & 1) * 4 + ((l >> 3) & 1) * 2 + ((l >> 2) & 1) of the wave
        if ((lane & 3u) == 0u) s_part[wave][((lane >> 5) & 1u) * 8u + ((lane >> 4) & 1u) * 4u + ((lane >> 3) & 1u) * 2u + ((lane >> 2) & 1u)] = acc[0];
        __syncthreads();
        if (t < EM_L) {
            double sum = s_part[0][t];
#pragma unroll
            for (uint32_t w = 1; w < EM_WAVES; w++) sum += s_part[w][t];
            double mine = 0.0;
#pragma unroll
            for (uint32_t j = 0; j < EM_L; j++) mine = t == j ? rho[j] : mine;
            const double next = mine * sum / N;
            s_rho[t] = next;
            s_delta[t] = fabs(next - mine);
        }
        __syncthreads();
        double delta = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < EM_L; j++) {
            rho[j] = s_rho[j];
            delta = fmax(delta, s_delta[j]);
        }
        it++;
        if (it >= max_iter || delta < tol) break;                   // (the same in every thread)
        // s_rho and s_delta are written again only behind the next iteration's first barrier, which every thread reaches after
        // it has read them
    }
    if (t < n_strains) out[t] = s_rho[t];
    if (t == 0) iters_out[blockIdx.x] = it;
}

std::atomic<uint64_t> g_em_calls{0};

}  // namespace

extern "C" {

int ss_em_strain_sets_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_em_calls.load();
    return SS_OK;
}

int ss_em_strain_sets(const uint64_t *counts, const uint16_t *masks, uint32_t n_sets, uint32_t n_strains, uint32_t n_vec, uint32_t max_iter,
                      double tol, double *rho, uint32_t *iters)
{
    if (!counts || !masks || !rho || !iters || n_sets < 1 || n_sets > 65535 || n_strains < 1 || n_strains > SS_STRAIN_SET_MAX || n_vec < 1 ||
        n_vec > SS_EM_VECTORS_MAX || max_iter < 1 || !(tol >= 0.0))
        return SS_EINVAL;
    {
        std::vector<uint8_t> seen(1u << n_strains, 0);
        for (uint32_t s = 0; s < n_sets; s++) {
            const uint32_t m = masks[s];
            if (!m || (m >> n_strains) || seen[m]) return SS_EINVAL;
            seen[m] = 1;
        }
    }
    g_em_calls.fetch_add(1);
    ss::PoolScratch scratch;
    unsigned long long *d_counts = nullptr;
    uint16_t *d_masks = nullptr;
    double *d_rho = nullptr;
    uint32_t *d_iters = nullptr;
    const size_t cells = (size_t)n_vec * n_sets;
    SS_HIP(scratch.get((void **)&d_counts, cells * 8));
    SS_HIP(scratch.get((void **)&d_masks, (size_t)n_sets * 2));
    SS_HIP(scratch.get((void **)&d_rho, (size_t)n_vec * n_strains * 8));
    SS_HIP(scratch.get((void **)&d_iters, (size_t)n_vec * 4));
    SS_HIP(ss::l2s::copy(d_counts, counts, cells * 8, hipMemcpyHostToDevice));
    SS_HIP(ss::l2s::copy(d_masks, masks, (size_t)n_sets * 2, hipMemcpyHostToDevice));
    if (n_sets <= SS_EM_LDS_SETS)
        hipLaunchKernelGGL(em_kernel<true>, dim3(n_vec), dim3(EM_THREADS), 0, ss::l2s::stream(), d_counts, d_masks, n_sets, n_strains, max_iter, tol,
                           d_rho, d_iters);
    else
        hipLaunchKernelGGL(em_kernel<false>, dim3(n_vec), dim3(EM_THREADS), 0, ss::l2s::stream(), d_counts, d_masks, n_sets, n_strains, max_iter, tol,
                           d_rho, d_iters);
    SS_HIP(hipGetLastError());
    SS_HIP(ss::l2s::copy(rho, d_rho, (size_t)n_vec * n_strains * 8, hipMemcpyDeviceToHost));
    SS_HIP(ss::l2s::copy(iters, d_iters, (size_t)n_vec * 4, hipMemcpyDeviceToHost));
    return SS_OK;
}

}  // extern "C"
