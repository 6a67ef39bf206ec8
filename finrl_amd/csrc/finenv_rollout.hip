// finenv_rollout.hip -- rollout-buffer helpers over [n_steps][E] tensors (gfx950): the GAE
// time-reverse scan, the one-launch store of a policy's outputs into slice t, and the shuffled
// minibatch -- a stateless permutation (Feistel rounds of Philox4x32-10, cycle-walked) and the gather
// of a row's six fields in one launch.
// GAE: one lane per env, fully coalesced row reads; float32 with the operation order of SB3's
// documented RolloutBuffer.compute_returns_and_advantage (see include/finenv.h).  HBM-bound:
// 17 bytes per (step, env).
// Minibatch: pure data movement behind 4 Philox calls per pass of the permutation: 4D read + 4D write
// + 8A + 36 bytes per sample with rows out.  No LDS, no barrier; every offset is 64-bit (the
// observation tensor passes 4 GiB at real shapes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "finenv.h"
#include "finenv_host.h"
#include "finenv_dev.h"
#include "finenv_group.h"       // f4, group_sample, philox4x32_10

namespace {
__global__ void __launch_bounds__(256) gae_scan_kernel(const float *__restrict__ rewards,
                                                       const float *__restrict__ values,
                                                       const uint8_t *__restrict__ dones,
                                                       const float *__restrict__ last_values,
                                                       float *__restrict__ adv,
                                                       float *__restrict__ ret, int S, int E,
                                                       float gamma, float lam)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    float next_v = last_values[e];
    float gae = 0.0f;
    const float gl = gamma * lam;
#pragma unroll 4
    for (int t = S - 1; t >= 0; --t) {
        const size_t k = (size_t)t * E + e;
        const float nnt = 1.0f - (float)dones[k];
        const float v = values[k];
        const float delta = rewards[k] + gamma * next_v * nnt - v;
        gae = delta + gl * nnt * gae;
        adv[k] = gae;
        ret[k] = gae + v;
        next_v = v;
    }
}

// actions [E*A], values [E], log-probs [E] -> slice t of the rollout tensors, one launch (three
// separate copy launches cost ~2 us each at 32,768 envs: more than the env step they sit beside)
template <typename V>
__global__ void __launch_bounds__(256) rollout_put_kernel(const V *__restrict__ a_src, V *__restrict__ a_dst,
                                                          const V *__restrict__ v_src, V *__restrict__ v_dst,
                                                          const V *__restrict__ l_src, V *__restrict__ l_dst,
                                                          int na, int nv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) {
        a_dst[i] = a_src[i];
    } else if (i < na + nv) {
        v_dst[i - na] = v_src[i - na];
    } else if (i < na + 2 * nv) {
        l_dst[i - na - nv] = l_src[i - na - nv];
    }
}

// The minibatch kernel's argument: the two ABI structs, the epoch word, and what the host derives
// from M = n_steps * n_envs (the half widths of the Feistel network).
struct MinibatchArgs {
    finenv_rollout_view v;
    finenv_rollout_batch o;
    const int64_t *epoch;         // the epoch number, read at each launch / replay
    int32_t *rows_out;            // [B] or NULL
    uint32_t seed_lo, seed_hi;
    uint32_t first;               // position of sample 0; first + B <= M < 2^31 (host-checked)
    uint32_t n_rows;              // M
    int32_t a_bits, b_bits;       // bits / 2 and bits - a_bits, bits = max(2, bit_length(M - 1))
};

// Position x of epoch (n_lo, n_hi) -> its row (contract: include/finenv.h, "Permutation").  The rounds
// are a bijection of [0, 2^bits) whatever the words hold, so the walk ends and the row is below M.
__device__ __forceinline__ uint32_t rollout_perm(const MinibatchArgs &a, uint32_t x, uint32_t n_lo,
                                                 uint32_t n_hi)
{
    if (a.n_rows == 1u) return 0u;
    const uint32_t ma = (1u << a.a_bits) - 1u, mb = (1u << a.b_bits) - 1u;
    do {
        uint32_t L = x >> a.a_bits, R = x & ma;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            uint32_t f, unused;
            philox4x32_10((r & 1u) ? L : R, r, n_lo, n_hi, a.seed_lo, a.seed_hi, f, unused);
            if (r & 1u)
                R ^= f & ma;
            else
                L ^= f & mb;
        }
        x = (L << a.a_bits) | R;
    } while (x >= a.n_rows);
    return x;
}

// One sample per group of G lanes (G = 64: per wave, with position and row made scalar, so the walk is
// uniform and the Philox rounds run on the scalar unit; below that the walk diverges inside a wave).
// The tensors are time-major and contiguous, so row r = t * E + e of every field sits at r times the
// field's row size: no division by E.  The form is the replay sampler's gather_rows with one row: the
// first two units per lane, the action row's first unit, the tail of D % 4 floats (f4 only) and the
// four scalar words -- lanes 0 .. 3 of the group take one each -- are all loaded before the first
// store (a load behind the wave's own stores waits for them); units past 2G and action
// floats past G go through the loops behind the stores.  Columns D .. pitch-1 of the output are never
// written.
template <int G, typename V>
__global__ void __launch_bounds__(256) rollout_minibatch_kernel(const MinibatchArgs a)
{
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    int lane;
    const long long b = group_sample<G>(lane);
    if (b >= a.o.batch_size) return;

    uint32_t i = a.first + (uint32_t)b;
    if (G == 64) i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
    const uint64_t n = (uint64_t)*a.epoch;
    uint32_t r = rollout_perm(a, i, (uint32_t)n, (uint32_t)(n >> 32));
    if (G == 64) r = (uint32_t)__builtin_amdgcn_readfirstlane((int)r);

    const int D = a.v.obs_dim, A = a.v.action_dim;
    const float *row = a.v.obs + (long long)r * a.v.obs_pitch;
    const float *arow = a.v.actions + (long long)r * A;
    float *out = a.o.observations + b * a.o.obs_pitch;
    float *aout = a.o.actions + b * A;
    const V *src = (const V *)row;
    V *dst = (V *)out;
    // lane j < 4 of the group moves scalar field j
    const float *sp = lane == 0 ? a.v.values : lane == 1 ? a.v.log_probs
                    : lane == 2 ? a.v.advantages : a.v.returns;
    float *dp = lane == 0 ? a.o.old_values : lane == 1 ? a.o.old_log_prob
              : lane == 2 ? a.o.advantages : a.o.returns;

    const int nu = D / VW;                    // whole units per row
    const int tail = D - nu * VW;             // f4: the last D % 4 floats
    const int k0 = lane, k1 = lane + G;
    const bool p0 = k0 < nu, p1 = k1 < nu, pa = lane < A, pt = VW > 1 && lane < tail, ps = lane < 4;
    V x0 = {}, x1 = {};
    float av = 0.0f, t0 = 0.0f, sv = 0.0f;
    if (p0) x0 = src[k0];
    if (p1) x1 = src[k1];
    if (pa) av = arow[lane];
    if (pt) t0 = row[nu * VW + lane];
    if (ps) sv = sp[r];
    if (p0) dst[k0] = x0;
    if (p1) dst[k1] = x1;
    if (pa) aout[lane] = av;
    if (pt) out[nu * VW + lane] = t0;
    if (ps) dp[b] = sv;
    if (lane == 0 && a.rows_out != nullptr) a.rows_out[b] = (int32_t)r;
    for (int k = lane + 2 * G; k < nu; k += G) dst[k] = src[k];
    for (int k = lane + G; k < A; k += G) aout[k] = arow[k];
}

// The launch for lane groups of G and 16-byte (vec) or dword units: 256 / G samples per block.
int launch_minibatch(int G, bool vec, const MinibatchArgs &args, void *stream)
{
    const auto launch = [&](auto g) {
        constexpr int GG = decltype(g)::value;
        const dim3 grid((unsigned)(((long long)args.o.batch_size * GG + 255) / 256));
        const auto kernel = vec ? &rollout_minibatch_kernel<GG, f4> : &rollout_minibatch_kernel<GG, float>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, args);
    };
    switch (G) {
    case 4: launch(std::integral_constant<int, 4>()); break;
    case 8: launch(std::integral_constant<int, 8>()); break;
    case 16: launch(std::integral_constant<int, 16>()); break;
    case 32: launch(std::integral_constant<int, 32>()); break;
    default: launch(std::integral_constant<int, 64>()); break;
    }
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
}
}  // namespace

extern "C" int finenv_rollout_put(const float *actions, const float *values, const float *log_probs,
                                  float *actions_out, float *values_out, float *log_probs_out,
                                  int32_t n_envs, int32_t action_dim, void *stream)
{
    if (!actions || !values || !log_probs || !actions_out || !values_out || !log_probs_out ||
        n_envs < 1 || action_dim < 1 || (long long)n_envs * action_dim > (1ll << 30))
        return FINENV_ERR_INVALID;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(actions_out));
    const int na = n_envs * action_dim, nv = n_envs;
    const uintptr_t bits = (uintptr_t)actions | (uintptr_t)values | (uintptr_t)log_probs |
                           (uintptr_t)actions_out | (uintptr_t)values_out | (uintptr_t)log_probs_out;
    if ((bits & 15) == 0 && (na & 3) == 0 && (nv & 3) == 0) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const int n4 = (na + 2 * nv) / 4;
        hipLaunchKernelGGL(rollout_put_kernel<f4>, dim3((n4 + 255) / 256), dim3(256), 0,
                           (hipStream_t)stream, (const f4 *)actions, (f4 *)actions_out,
                           (const f4 *)values, (f4 *)values_out, (const f4 *)log_probs,
                           (f4 *)log_probs_out, na / 4, nv / 4);
    } else {
        const int n = na + 2 * nv;
        hipLaunchKernelGGL(rollout_put_kernel<float>, dim3((n + 255) / 256), dim3(256), 0,
                           (hipStream_t)stream, actions, actions_out, values, values_out, log_probs,
                           log_probs_out, na, nv);
    }
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
}

extern "C" int finenv_gae_scan(const float *rewards, const float *values, const uint8_t *dones,
                               const float *last_values, float *advantages, float *returns,
                               int32_t n_steps, int32_t n_envs, float gamma, float gae_lambda,
                               void *stream)
{
    if (!rewards || !values || !dones || !last_values || !advantages || !returns ||
        n_steps < 1 || n_envs < 1)
        return FINENV_ERR_INVALID;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(rewards));
    hipLaunchKernelGGL(gae_scan_kernel, dim3((n_envs + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, rewards, values, dones, last_values, advantages,
                       returns, n_steps, n_envs, gamma, gae_lambda);
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
}

extern "C" int finenv_rollout_minibatch(const finenv_rollout_view *view, const int64_t *epoch,
                                        uint64_t seed, int64_t first, const finenv_rollout_batch *batch,
                                        int32_t *rows_out, void *stream)
{
    if (!view || !batch || !epoch) return FINENV_ERR_INVALID;
    const finenv_rollout_view &v = *view;
    const finenv_rollout_batch &o = *batch;
    if (!v.obs || !v.actions || !v.values || !v.log_probs || !v.advantages || !v.returns ||
        !o.observations || !o.actions || !o.old_values || !o.old_log_prob || !o.advantages || !o.returns)
        return FINENV_ERR_INVALID;
    if (v.n_steps < 1 || v.n_envs < 1 || v.obs_dim < 1 || v.action_dim < 1 || v.obs_pitch < v.obs_dim ||
        o.batch_size < 1 || o.obs_pitch < v.obs_dim)
        return FINENV_ERR_INVALID;
    const long long M = (long long)v.n_steps * v.n_envs;
    if (M > 0x7fffffffLL || first < 0 || first > M - o.batch_size) return FINENV_ERR_INVALID;

    // the row path and the lane group: the replay sampler's rule (gather_group of finenv_replay.hip)
    // over the two observation bases
    const uintptr_t bits = (uintptr_t)v.obs | (uintptr_t)o.observations;
    const bool vec = (bits & 15) == 0 && (v.obs_pitch & 3) == 0 && (o.obs_pitch & 3) == 0 && v.obs_dim >= 4;
    const int units = vec ? (v.obs_dim + 3) / 4 : v.obs_dim;
    int G = 4;
    while (G < 64 && 2 * G < units) G *= 2;

    int nbits = 0;                                // bit_length(M - 1)
    while (nbits < 31 && ((M - 1) >> nbits) != 0) ++nbits;
    nbits = nbits < 2 ? 2 : nbits;
    const MinibatchArgs args = {v, o, epoch, rows_out, (uint32_t)seed, (uint32_t)(seed >> 32),
                                (uint32_t)first, (uint32_t)M, nbits / 2, nbits - nbits / 2};
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(o.observations));
    return launch_minibatch(G, vec, args, stream);
}
