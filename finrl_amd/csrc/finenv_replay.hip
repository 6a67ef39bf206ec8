// finenv_replay.hip -- replay buffer for the off-policy agents (gfx950): the one-launch store of a
// step's actions plus the ring head, and the sampler -- draw (slot, env) pairs with Philox4x32-10 or
// take the caller's, then gather obs / next_obs / action / reward / done rows into a batch.  Contract:
// include/finenv.h.  Pure data movement, HBM/L2-bound: 2 * (4D read + 4D write) + 8A + 21 bytes per
// sample (indices_out: + 8).  No LDS, no barrier; every offset is 64-bit (the ring may pass 4 GiB).
// The n-step form (replay_nstep_kernel) adds the h reward / done words of a pair's window and the
// discount: + 5h + 4 bytes per sample, and a second round trip for the late next-observation row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "finenv.h"
#include "finenv_host.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

// actions -> their ring slot, and the head words after this step (set, never incremented: a replayed
// capture publishes the head of the slots it writes)
template <typename V>
__global__ void __launch_bounds__(256) replay_put_kernel(const V *src, V *dst, int n, int32_t *head,
                                                         int32_t pos_next, int32_t n_valid_next)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
    if (i == 0) {
        head[0] = pos_next;
        head[1] = n_valid_next;
    }
}

struct GatherArgs {
    finenv_replay_view v;
    finenv_replay_batch o;
    const int32_t *head;          // DRAW: {pos, n_valid}
    const int64_t *draw;          // DRAW: the draw number
    const int32_t *indices;       // !DRAW: [2][B]
    int32_t *indices_out;         // DRAW: [2][B] or NULL
    uint32_t seed_lo, seed_hi;
};

// Philox4x32-10 (Salmon et al., SC'11; Random123): counter c[4], key k[2] -> first two output words
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t &x0, uint32_t &x1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x0 = c0;
    x1 = c1;
}

// The clamped (slot, env) of sample b -> s, e; returns its age, the stored steps between it and the
// newest.  DRAW: the Philox words give an age below n_valid (not trusted: clamped into [1, S - 1]) and
// an env below E; the slot is (pos - 1 - age) mod S, never slot pos of a full ring.  !DRAW: the
// caller's indices, clamped, and the age from (pos - 1 - s) mod S.  G = 64: (slot, env) is made scalar,
// so the row bases are.  A kernel that ignores the age loses it and, !DRAW, the head load when compiled.
template <int G, bool DRAW>
__device__ __forceinline__ int sample_pair(const GatherArgs &a, long long b, int &s, int &e)
{
    const int S = a.v.n_slots, E = a.v.n_envs;
    const int32_t pos = a.head[0];
    long long age;
    if (DRAW) {
        int32_t nv = a.head[1];
        nv = nv < 1 ? 1 : (nv > S - 1 ? S - 1 : nv);
        const uint64_t draw = (uint64_t)*a.draw;
        uint32_t x0, x1;
        philox4x32_10((uint32_t)b, 0u, (uint32_t)draw, (uint32_t)(draw >> 32), a.seed_lo, a.seed_hi,
                      x0, x1);
        age = (long long)__umulhi(x0, (uint32_t)nv);
        const long long q = ((long long)pos - 1 - age) % S;
        s = (int)(q < 0 ? q + S : q);
        e = (int)__umulhi(x1, (uint32_t)E);
    } else {
        s = a.indices[b];
        e = a.indices[(long long)a.o.batch_size + b];
        s = s < 0 ? 0 : (s > S - 1 ? S - 1 : s);
        e = e < 0 ? 0 : (e > E - 1 ? E - 1 : e);
        const long long q = ((long long)pos - 1 - s) % S;
        age = q < 0 ? q + S : q;
    }
    if (G == 64) {
        s = __builtin_amdgcn_readfirstlane(s);
        e = __builtin_amdgcn_readfirstlane(e);
    }
    return (int)age;
}

// What the kernels' up-front loads leave: the units past 2G of both rows and the action floats past G,
// behind the wave's stores (none of the shipped env shapes at their G has either).
template <int G, typename V>
__device__ __forceinline__ void copy_rest(const V *src0, const V *src1, V *dst0, V *dst1, int nu,
                                          const float *arow, float *aout, int A, int lane)
{
    for (int k = lane + 2 * G; k < nu; k += G) {
        const V x = src0[k], y = src1[k];
        dst0[k] = x;
        dst1[k] = y;
    }
    for (int k = lane + G; k < A; k += G) aout[k] = arow[k];
}

// The one-step sampler: one sample per group of G lanes (G = 64: per wave).  A row is `nu` units of V
// (f4 where pitches and bases allow, else float) plus, for f4, a tail of D % 4 floats moved as dwords:
// columns D .. pitch-1 of the outputs are never written.  The first two units per lane of both rows,
// the action row's first unit, the tail and the reward / done words are all loaded before the first
// store -- a load behind the wave's own stores waits for them.  The two rows alternate
// unit by unit: one row after the other measured 4 % slower (profiles/replay_share.md).
template <int G, typename V, bool DRAW>
__global__ void __launch_bounds__(256) replay_gather_kernel(const GatherArgs a)
{
    constexpr int PER_BLOCK = 256 / G;
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    const int lane = (int)threadIdx.x & (G - 1);
    const long long b = (long long)blockIdx.x * PER_BLOCK + ((int)threadIdx.x / G);
    const int B = a.o.batch_size;
    if (b >= B) return;
    const int S = a.v.n_slots, E = a.v.n_envs, D = a.v.obs_dim, A = a.v.action_dim;

    int s, e;
    sample_pair<G, DRAW>(a, b, s, e);             // the age is not needed: one step ends at the newest
    if (DRAW && a.indices_out != nullptr && lane == 0) {
        a.indices_out[b] = s;
        a.indices_out[(long long)B + b] = e;
    }
    const int s1 = s + 1 == S ? 0 : s + 1;
    const long long se = (long long)s * E + e, se1 = (long long)s1 * E + e;
    const float *row0 = a.v.obs + se * a.v.obs_pitch;
    const float *row1 = a.v.obs + se1 * a.v.obs_pitch;
    const float *arow = a.v.actions + se * A;
    float *out0 = a.o.observations + b * a.o.obs_pitch;
    float *out1 = a.o.next_observations + b * a.o.obs_pitch;
    float *aout = a.o.actions + b * A;
    const V *src0 = (const V *)row0, *src1 = (const V *)row1;
    V *dst0 = (V *)out0, *dst1 = (V *)out1;

    const int nu = D / VW;                    // whole units per row
    const int tail = D - nu * VW;             // f4: the last D % 4 floats
    const int k0 = lane, k1 = lane + G;
    const bool p0 = k0 < nu, p1 = k1 < nu, pa = lane < A, pt = VW > 1 && lane < tail;
    V x0 = {}, x1 = {}, y0 = {}, y1 = {};
    float av = 0.0f, t0 = 0.0f, t1 = 0.0f, rew = 0.0f;
    uint8_t dn = 0;
    if (p0) {
        x0 = src0[k0];
        y0 = src1[k0];
    }
    if (p1) {
        x1 = src0[k1];
        y1 = src1[k1];
    }
    if (pa) av = arow[lane];
    if (pt) {
        t0 = row0[nu * VW + lane];
        t1 = row1[nu * VW + lane];
    }
    if (lane == 0) {
        rew = a.v.rewards[se];
        dn = a.v.dones[se];
    }
    if (p0) {
        dst0[k0] = x0;
        dst1[k0] = y0;
    }
    if (p1) {
        dst0[k1] = x1;
        dst1[k1] = y1;
    }
    if (pa) aout[lane] = av;
    if (pt) {
        out0[nu * VW + lane] = t0;
        out1[nu * VW + lane] = t1;
    }
    if (lane == 0) {
        a.o.rewards[b] = rew;
        a.o.dones[b] = (float)dn;
    }
    copy_rest<G, V>(src0, src1, dst0, dst1, nu, arow, aout, A, lane);
}

struct NStepArgs {
    GatherArgs g;                 // head is read in both forms: the horizon ends at the newest step
    float *discounts;             // [B]
    int32_t *steps;               // [B] or NULL
    int32_t n_steps;
    float gamma;
};

// The n-step sampler (contract: include/finenv.h, "n-step returns"): sample_pair, copy_rest and the
// units per lane are those of replay_gather_kernel; what differs is that the next-observation row is
// known only after the return's length m.  Round trip 1: lane i of the group loads the reward and done
// words of step i of the window (slot (s+i) mod S, i < h = min(age + 1, n)), beside the observation
// row of s and the action row.  Then m by a ballot over the group's done words, the sum in the stated
// order (every lane of the group forms it, from shuffled rewards), round trip 2 for the row of slot
// (s+m) mod S, and only then the stores, the drawn pair among them: a load behind the wave's own
// stores waits for them.  n > G (only the narrow groups of short rows) takes one more
// round trip per further chunk of G steps.  All control flow but the loads' and stores' predicates is
// uniform over the launch, so the ballot and the shuffles see every lane of a live group.  h <= n <=
// S - 1 (host-checked) keeps every slot below 2S before its one conditional subtract.
template <int G, typename V, bool DRAW>
__global__ void __launch_bounds__(256) replay_nstep_kernel(const NStepArgs na)
{
    const GatherArgs &a = na.g;
    constexpr int PER_BLOCK = 256 / G;
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    const int lane = (int)threadIdx.x & (G - 1);
    const long long b = (long long)blockIdx.x * PER_BLOCK + ((int)threadIdx.x / G);
    const int B = a.o.batch_size;
    if (b >= B) return;
    const int S = a.v.n_slots, E = a.v.n_envs, D = a.v.obs_dim, A = a.v.action_dim;
    const int n = na.n_steps;
    const float gamma = na.gamma;

    int s, e;
    const int age = sample_pair<G, DRAW>(a, b, s, e);
    int h = age + 1 < n ? age + 1 : n;            // the horizon ends at the newest step
    if (G == 64) h = __builtin_amdgcn_readfirstlane(h);
    const long long se = (long long)s * E + e;
    const float *row0 = a.v.obs + se * a.v.obs_pitch;
    const float *arow = a.v.actions + se * A;
    float *out0 = a.o.observations + b * a.o.obs_pitch;
    float *out1 = a.o.next_observations + b * a.o.obs_pitch;
    float *aout = a.o.actions + b * A;
    const V *src0 = (const V *)row0;
    V *dst0 = (V *)out0, *dst1 = (V *)out1;

    const int nu = D / VW;
    const int tail = D - nu * VW;
    const int k0 = lane, k1 = lane + G;
    const bool p0 = k0 < nu, p1 = k1 < nu, pa = lane < A, pt = VW > 1 && lane < tail;
    V x0 = {}, x1 = {}, y0 = {}, y1 = {};
    float av = 0.0f, t0 = 0.0f, t1 = 0.0f, rew = 0.0f;
    uint8_t dn = 0;
    // round trip 1
    if (p0) x0 = src0[k0];
    if (p1) x1 = src0[k1];
    if (pa) av = arow[lane];
    if (pt) t0 = row0[nu * VW + lane];
    if (lane < h) {
        int sw = s + lane;
        sw = sw >= S ? sw - S : sw;
        const long long w = (long long)sw * E + e;
        rew = a.v.rewards[w];
        dn = a.v.dones[w];
    }

    const int gshift = ((int)threadIdx.x & 63) & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
    double acc = 0.0;
    float g = 1.0f, dlast = 0.0f;
    int m = 0;
    bool open = true;                             // neither a done nor the horizon reached yet
    for (int base = 0; base < n; base += G) {
        if (base > 0) {                           // n > G: the next chunk of the window
            rew = 0.0f;
            dn = 0;
            if (open && base + lane < h) {
                int sw = s + base + lane;
                sw = sw >= S ? sw - S : sw;
                const long long w = (long long)sw * E + e;
                rew = a.v.rewards[w];
                dn = a.v.dones[w];
            }
        }
        const int cnt = h - base < G ? h - base : G;       // steps of the window in this chunk
        const unsigned long long hit = (__ballot(dn != 0) >> gshift) & gmask;
        const int k = hit ? __builtin_ctzll(hit) : cnt - 1; // the chunk's last step of the return
        const int lim = n - base < G ? n - base : G;
        for (int i = 0; i < lim; ++i) {
            const float ri = __shfl(rew, i, G);
            const bool on = open && i <= k;
            const double t = (double)g * (double)ri;
            acc = on ? (base + i == 0 ? t : acc + t) : acc;
            g = on ? g * gamma : g;
        }
        const float dk = (float)__shfl((int)dn, k & (G - 1), G);
        if (open && cnt > 0) {
            m = base + k + 1;
            dlast = dk;
            open = hit == 0 && m < h;
        }
    }
    if (G == 64) m = __builtin_amdgcn_readfirstlane(m);

    // round trip 2: the row of slot (s + m) mod S
    int s1 = s + m;
    s1 = s1 >= S ? s1 - S : s1;
    const float *row1 = a.v.obs + ((long long)s1 * E + e) * a.v.obs_pitch;
    const V *src1 = (const V *)row1;
    if (p0) y0 = src1[k0];
    if (p1) y1 = src1[k1];
    if (pt) t1 = row1[nu * VW + lane];

    if (p0) {
        dst0[k0] = x0;
        dst1[k0] = y0;
    }
    if (p1) {
        dst0[k1] = x1;
        dst1[k1] = y1;
    }
    if (pa) aout[lane] = av;
    if (pt) {
        out0[nu * VW + lane] = t0;
        out1[nu * VW + lane] = t1;
    }
    if (lane == 0) {
        a.o.rewards[b] = (float)acc;
        a.o.dones[b] = dlast;
        na.discounts[b] = g;
        if (na.steps != nullptr) na.steps[b] = m;
        if (DRAW && a.indices_out != nullptr) {   // with the other stores, not ahead of the loads
            a.indices_out[b] = s;
            a.indices_out[(long long)B + b] = e;
        }
    }
    copy_rest<G, V>(src0, src1, dst0, dst1, nu, arow, aout, A, lane);
}

// The kernels are function templates: a functor each names the instantiation for the launcher.
struct GatherKernel {
    template <int G, typename V, bool DRAW>
    static constexpr auto get() { return &replay_gather_kernel<G, V, DRAW>; }
};
struct NStepKernel {
    template <int G, typename V, bool DRAW>
    static constexpr auto get() { return &replay_nstep_kernel<G, V, DRAW>; }
};

// One launch of K's kernel for lane groups of G and 16-byte (vec) or dword units: 256 / G samples per
// block, on the device of the batch.
template <typename K, bool DRAW, typename Args>
int launch_sampler(int G, bool vec, const Args &args, const finenv_replay_batch &o, void *stream)
{
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(o.observations));
    const auto launch = [&](auto g) {
        constexpr int GG = decltype(g)::value;
        const dim3 grid((unsigned)(((long long)o.batch_size * GG + 255) / 256));
        const auto kernel = vec ? K::template get<GG, f4, DRAW>() : K::template get<GG, float, DRAW>();
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

// Shape checks of the two structs (no HIP call before they pass), then the row path and the lane
// group: 16-byte units when the pitches and the three bases allow, and the smallest power of two in
// [4, 64] that covers a row with the two units a lane loads up front -- a 3-unit row takes 4 lanes, a
// 51-dword crypto row half a wave, the 76 units of a DOW30 row a whole one.  Returns the group width
// (and whether the units are 16 bytes), or 0 for a shape that is refused.
int gather_group(const finenv_replay_view &v, const finenv_replay_batch &o, bool &vec)
{
    if (!v.obs || !v.actions || !v.rewards || !v.dones || !o.observations || !o.next_observations ||
        !o.actions || !o.rewards || !o.dones)
        return 0;
    if (v.n_slots < 2 || v.n_envs < 1 || v.obs_dim < 1 || v.action_dim < 1 || v.obs_pitch < v.obs_dim ||
        o.batch_size < 1 || o.obs_pitch < v.obs_dim)
        return 0;
    const uintptr_t bits = (uintptr_t)v.obs | (uintptr_t)o.observations | (uintptr_t)o.next_observations;
    vec = (bits & 15) == 0 && (v.obs_pitch & 3) == 0 && (o.obs_pitch & 3) == 0 && v.obs_dim >= 4;
    const int units = vec ? (v.obs_dim + 3) / 4 : v.obs_dim;
    int G = 4;
    while (G < 64 && 2 * G < units) G *= 2;
    return G;
}

template <bool DRAW>
int launch_gather(const GatherArgs &a, void *stream)
{
    bool vec = false;
    const int G = gather_group(a.v, a.o, vec);
    if (G == 0) return FINENV_ERR_INVALID;
    return launch_sampler<GatherKernel, DRAW>(G, vec, a, a.o, stream);
}

// The n-step launch: the gather's checks, then 1 <= n_steps <= S - 1 (a window never reaches round
// to its own start), gamma finite in [0, 1], head and discounts present.
template <bool DRAW>
int launch_nstep(GatherArgs a, const finenv_replay_nstep *ns, void *stream)
{
    bool vec = false;
    const int G = gather_group(a.v, a.o, vec);
    if (G == 0 || !ns->head || !ns->discounts || ns->n_steps < 1 || ns->n_steps > a.v.n_slots - 1 ||
        !(ns->gamma >= 0.0f && ns->gamma <= 1.0f))
        return FINENV_ERR_INVALID;
    if (!DRAW) a.head = ns->head;
    const NStepArgs na = {a, ns->discounts, ns->steps, ns->n_steps, ns->gamma};
    return launch_sampler<NStepKernel, DRAW>(G, vec, na, a.o, stream);
}

// The kernel arguments of a drawn call and of a call with the caller's indices.
GatherArgs drawn_args(const finenv_replay_view *view, const finenv_replay_batch *batch,
                      const int32_t *head, const int64_t *draw, uint64_t seed, int32_t *indices_out)
{
    return {*view, *batch, head, draw, nullptr, indices_out, (uint32_t)seed, (uint32_t)(seed >> 32)};
}

GatherArgs index_args(const finenv_replay_view *view, const finenv_replay_batch *batch,
                      const int32_t *indices)
{
    return {*view, *batch, nullptr, nullptr, indices, nullptr, 0u, 0u};
}

}  // namespace

extern "C" int finenv_replay_put(const float *actions, float *actions_slot, int32_t n_floats,
                                 int32_t *head, int32_t pos_next, int32_t n_valid_next, void *stream)
{
    if (!actions || !actions_slot || !head || n_floats < 1 || n_floats > (1 << 30) || pos_next < 0 ||
        n_valid_next < 0)
        return FINENV_ERR_INVALID;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(actions_slot));
    if ((((uintptr_t)actions | (uintptr_t)actions_slot) & 15) == 0 && (n_floats & 3) == 0) {
        const int n4 = n_floats / 4;
        hipLaunchKernelGGL(replay_put_kernel<f4>, dim3((n4 + 255) / 256), dim3(256), 0,
                           (hipStream_t)stream, (const f4 *)actions, (f4 *)actions_slot, n4, head,
                           pos_next, n_valid_next);
    } else {
        hipLaunchKernelGGL(replay_put_kernel<float>, dim3((n_floats + 255) / 256), dim3(256), 0,
                           (hipStream_t)stream, actions, actions_slot, n_floats, head, pos_next,
                           n_valid_next);
    }
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
}

extern "C" int finenv_replay_sample(const finenv_replay_view *view, const int32_t *head,
                                    const int64_t *draw, uint64_t seed,
                                    const finenv_replay_batch *batch, int32_t *indices_out, void *stream)
{
    if (!view || !batch || !head || !draw) return FINENV_ERR_INVALID;
    return launch_gather<true>(drawn_args(view, batch, head, draw, seed, indices_out), stream);
}

extern "C" int finenv_replay_gather(const finenv_replay_view *view, const int32_t *indices,
                                    const finenv_replay_batch *batch, void *stream)
{
    if (!view || !batch || !indices) return FINENV_ERR_INVALID;
    return launch_gather<false>(index_args(view, batch, indices), stream);
}

extern "C" int finenv_replay_sample_nstep(const finenv_replay_view *view, const int32_t *head,
                                          const int64_t *draw, uint64_t seed,
                                          const finenv_replay_batch *batch,
                                          const finenv_replay_nstep *nstep, int32_t *indices_out,
                                          void *stream)
{
    if (!view || !batch || !head || !draw || !nstep) return FINENV_ERR_INVALID;
    return launch_nstep<true>(drawn_args(view, batch, head, draw, seed, indices_out), nstep, stream);
}

extern "C" int finenv_replay_gather_nstep(const finenv_replay_view *view, const int32_t *indices,
                                          const finenv_replay_batch *batch,
                                          const finenv_replay_nstep *nstep, void *stream)
{
    if (!view || !batch || !indices || !nstep) return FINENV_ERR_INVALID;
    return launch_nstep<false>(index_args(view, batch, indices), nstep, stream);
}
