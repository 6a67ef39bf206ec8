// finenv_replay.hip -- replay buffer for the off-policy agents (gfx950): the one-launch store of a
// step's actions plus the ring head, and the sampler -- draw (slot, env) pairs with Philox4x32-10 or
// take the caller's, then gather obs / next_obs / action / reward / done rows into a batch.  Contract:
// include/finenv.h.  Pure data movement, HBM/L2-bound: 2 * (4D read + 4D write) + 8A + 21 bytes per
// sample (indices_out: + 8).  No LDS, no barrier; every offset is 64-bit (the ring may pass 4 GiB).
// The n-step form (nstep_rows) adds the h reward / done words of a pair's window and the discount:
// + 5h + 4 bytes per sample, and a second round trip for the late next-observation row.
// Prioritised replay (per_*) keeps uint32 tickets and a fan-out-64 tree of exact uint64 sums beside
// the ring; its proportional draw costs one round trip per tree level.
// One sampler kernel, replay_sample_kernel<G, V, Draw, Args>: a draw source (UniformDraw, CallerDraw
// or TicketDraw) yields the pair, the return form (Args: GatherArgs or NStepArgs) moves the rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "finenv.h"
#include "finenv_host.h"
#include "finenv_group.h"       // f4, group_sample, philox4x32_10

namespace {

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

// The row arguments and the words a draw reads (the parent layout of the kernel's first argument: the
// scalar argument loads of every form stay where they were)
struct GatherArgs {
    finenv_replay_view v;
    finenv_replay_batch o;
    const int32_t *head;          // {pos, n_valid}: the uniform draw, and the age of the n-step forms
    const int64_t *draw;          // the draw number of the uniform and the ticket draw
    const int32_t *indices;       // the caller's pairs [2][B]
    int32_t *indices_out;         // the drawn pairs [2][B] or NULL
    uint32_t seed_lo, seed_hi;
};

// __ballot(pred) of this thread's group of G lanes, in bits 0 .. G-1
template <int G>
__device__ __forceinline__ unsigned long long group_ballot(bool pred)
{
    const int gshift = ((int)threadIdx.x & 63) & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
    return (__ballot(pred) >> gshift) & gmask;
}

// 64 values -> op over all of them, in every lane
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T x, Op op)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = op(x, (T)__shfl_xor(x, d, 64));
    return x;
}

// A caller's (slot, env), clamped into the ring
__device__ __forceinline__ void clamp_pair(int &s, int &e, int S, int E)
{
    s = s < 0 ? 0 : (s > S - 1 ? S - 1 : s);
    e = e < 0 ? 0 : (e > E - 1 ? E - 1 : e);
}

// (pos - 1 - x) mod S: the age of slot x, the stored steps between it and the newest -- and, the map
// being its own inverse, the slot of age x
__device__ __forceinline__ int steps_behind(int32_t pos, long long x, int S)
{
    const long long q = ((long long)pos - 1 - x) % S;
    return (int)(q < 0 ? q + S : q);
}

// leaf s * E + e of the ticket array -> s, e
__device__ __forceinline__ void leaf_pair(long long leaf, int E, int &s, int &e)
{
    s = (int)(leaf / E);
    e = (int)(leaf - (long long)s * E);
}

// The random words of sample b: Philox counter (b, 0, draw number), key = the seed
__device__ __forceinline__ void sample_words(const GatherArgs &a, long long b, uint32_t &x0, uint32_t &x1)
{
    const uint64_t n = (uint64_t)*a.draw;
    philox4x32_10((uint32_t)b, 0u, (uint32_t)n, (uint32_t)(n >> 32), a.seed_lo, a.seed_hi, x0, x1);
}

// (s, e) of sample b -> the index block ([2][B] or NULL)
__device__ __forceinline__ void store_pair(int32_t *out, long long b, int B, int s, int e)
{
    if (out != nullptr) {
        out[b] = s;
        out[(long long)B + b] = e;
    }
}

// What a draw source yields for sample b: the clamped pair, the age of its slot where the n-step form
// asks (NSTEP), and the probability of a ticket draw.
struct Drawn {
    int s, e, age;
    float prob;
};

// G = 64: (slot, env) is made scalar, so the row bases are
template <int G>
__device__ __forceinline__ void scalar_pair(Drawn &d)
{
    if (G == 64) {
        d.s = __builtin_amdgcn_readfirstlane(d.s);
        d.e = __builtin_amdgcn_readfirstlane(d.e);
    }
}

// The uniform draw from the head words {pos, n_valid}: the Philox words give an age below n_valid (not
// trusted: clamped into [1, S - 1]) and an env below E; the slot is the one of that age, never slot
// pos of a full ring.  Publishes the pair to indices_out -- in the one-step form straight away: held
// across the row loads it costs the groups below a wave 2 VGPRs.
struct UniformDraw {
    template <int G, bool NSTEP>
    __device__ __forceinline__ Drawn pair(const GatherArgs &a, long long b, int lane) const
    {
        const int S = a.v.n_slots, B = a.o.batch_size;
        const int32_t pos = a.head[0];
        int32_t nv = a.head[1];
        nv = nv < 1 ? 1 : (nv > S - 1 ? S - 1 : nv);
        uint32_t x0, x1;
        sample_words(a, b, x0, x1);
        Drawn d = {};
        const uint32_t age = __umulhi(x0, (uint32_t)nv);
        d.age = (int)age;
        d.s = steps_behind(pos, age, S);
        d.e = (int)__umulhi(x1, (uint32_t)a.v.n_envs);
        scalar_pair<G>(d);
        if (!NSTEP && lane == 0) store_pair(a.indices_out, b, B, d.s, d.e);
        return d;
    }
    template <bool NSTEP>
    __device__ __forceinline__ void publish(const GatherArgs &a, const Drawn &d, long long b) const
    {
        if (NSTEP) store_pair(a.indices_out, b, a.o.batch_size, d.s, d.e);
    }
};

// The caller's pairs, clamped; head is read only for the age.  Nothing to publish.
struct CallerDraw {
    template <int G, bool NSTEP>
    __device__ __forceinline__ Drawn pair(const GatherArgs &a, long long b, int) const
    {
        Drawn d = {};
        d.s = a.indices[b];
        d.e = a.indices[(long long)a.o.batch_size + b];
        clamp_pair(d.s, d.e, a.v.n_slots, a.v.n_envs);
        if (NSTEP) d.age = steps_behind(a.head[0], d.s, a.v.n_slots);
        scalar_pair<G>(d);
        return d;
    }
    template <bool NSTEP>
    __device__ __forceinline__ void publish(const GatherArgs &, const Drawn &, long long) const {}
};

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

// The one-step rows: one sample per group of G lanes (G = 64: per wave).  A row is `nu` units of V
// (f4 where pitches and bases allow, else float) plus, for f4, a tail of D % 4 floats moved as dwords:
// columns D .. pitch-1 of the outputs are never written.  The first two units per lane of both rows,
// the action row's first unit, the tail and the reward / done words are all loaded before the first
// store -- a load behind the wave's own stores waits for them.  The two rows alternate
// unit by unit: one row after the other measured 4 % slower (profiles/replay_share.md).
// `last` runs on the group's lane 0 with the reward / done stores: what the draw publishes.
template <int G, typename V, typename Last>
__device__ __forceinline__ void gather_rows(const GatherArgs &a, long long b, int lane, int s, int e,
                                            const Last &last)
{
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    const int S = a.v.n_slots, E = a.v.n_envs, D = a.v.obs_dim, A = a.v.action_dim;
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
        last();
    }
    copy_rest<G, V>(src0, src1, dst0, dst1, nu, arow, aout, A, lane);
}

struct NStepArgs : GatherArgs {
    float *discounts;             // [B]
    int32_t *steps;               // [B] or NULL
    int32_t n_steps;
    float gamma;
};

// The n-step rows (contract: include/finenv.h, "n-step returns"): copy_rest and the units per lane are
// those of gather_rows; what differs is that the next-observation row is known only after the return's
// length m.  Round trip 1: lane i of the group loads the reward and done
// words of step i of the window (slot (s+i) mod S, i < h = min(age + 1, n)), beside the observation
// row of s and the action row.  Then m by a ballot over the group's done words, the sum in the stated
// order (every lane of the group forms it, from shuffled rewards), round trip 2 for the row of slot
// (s+m) mod S, and only then the stores, the drawn pair among them: a load behind the wave's own
// stores waits for them.  n > G (only the narrow groups of short rows) takes one more
// round trip per further chunk of G steps.  All control flow but the loads' and stores' predicates is
// uniform over the launch, so the ballot and the shuffles see every lane of a live group.  h <= n <=
// S - 1 (host-checked) keeps every slot below 2S before its one conditional subtract.
template <int G, typename V, typename Last>
__device__ __forceinline__ void nstep_rows(const NStepArgs &na, long long b, int lane, int s, int e,
                                           int age, const Last &last)
{
    const GatherArgs &a = na;
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    const int S = a.v.n_slots, E = a.v.n_envs, D = a.v.obs_dim, A = a.v.action_dim;
    const int n = na.n_steps;
    const float gamma = na.gamma;

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
        const unsigned long long hit = group_ballot<G>(dn != 0);
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
        last();
    }
    copy_rest<G, V>(src0, src1, dst0, dst1, nu, arow, aout, A, lane);
}

// ------------------------------------------------------------------------------------------------
// Prioritised replay (contract: include/finenv.h, "Prioritised replay"): uint32 tickets per
// transition, a fan-out-64 tree of exact uint64 sums stored top-down, and the descent that turns a
// value u in [0, total) into the leaf whose ticket interval holds it.
// ------------------------------------------------------------------------------------------------
constexpr int PER_MAX_LEVELS = 6;         // 64^5 < 2^31 - 1 <= 64^6

// The tree of N leaves: cnt[0] = N, cnt[k] = nodes of level k = ceil(cnt[k-1] / 64), levels = the k
// with cnt[k] == 1; level k starts at word off[k] (off[levels] = 0: the root comes first).
struct PerTree {
    uint32_t *tickets;
    uint64_t *tree;
    int32_t levels;
    long long cnt[PER_MAX_LEVELS + 1];
    long long off[PER_MAX_LEVELS + 1];
};

// ticket of a shaped priority: 1 unless w > 0, else rint(w * 2^F) in double (exact), in [1, 2^32 - 1]
__device__ __forceinline__ uint32_t per_ticket(float w, int frac_bits)
{
    if (!(w > 0.0f)) return 1u;
    double x = rint((double)w * (double)(1ull << frac_bits));
    x = x < 1.0 ? 1.0 : (x > 4294967295.0 ? 4294967295.0 : x);
    return (uint32_t)x;
}

// 64 values -> their sum in every lane
__device__ __forceinline__ uint64_t wave_sum(uint64_t x)
{
    return (uint64_t)wave_reduce((unsigned long long)x, [](auto p, auto q) { return p + q; });
}

// One level of sums: a wave per node, out[node] = the sum of in[64 node .. 64 node + 63] below n_in.
template <typename T>
__global__ void __launch_bounds__(256) per_sum_kernel(const T *in, long long n_in, uint64_t *out,
                                                      long long n_out)
{
    const long long node = (long long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (node >= n_out) return;
    const long long i = node * 64 + ((int)threadIdx.x & 63);
    const uint64_t sum = wave_sum(i < n_in ? (uint64_t)in[i] : 0ull);
    if (((int)threadIdx.x & 63) == 0) out[node] = sum;
}

// The fill rule and level 1 under it: a wave per level-1 node of the two runs [a0, a0 + na) and
// [b0, b0 + nb) (disjoint: the host merges runs that meet).  Leaves in [fill0, fill1) take the
// largest ticket seen, leaves in [zero0, zero1) take 0, the rest stay; the wave owns its node, so
// the node is a plain store of the new sum.
__global__ void __launch_bounds__(256) per_put_kernel(uint32_t *tickets, uint64_t *level1,
                                                      long long n_leaves, const uint32_t *max_ticket,
                                                      long long fill0, long long fill1, long long zero0,
                                                      long long zero1, long long a0, long long na,
                                                      long long b0, long long nb)
{
    const long long w = (long long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (w >= na + nb) return;
    const long long node = w < na ? a0 + w : b0 + (w - na);
    const long long i = node * 64 + ((int)threadIdx.x & 63);
    uint32_t top = *max_ticket;
    top = top == 0u ? 1u : top;
    uint32_t q = 0u;
    if (i < n_leaves) {
        const bool fill = i >= fill0 && i < fill1, zero = i >= zero0 && i < zero1;
        q = fill ? top : (zero ? 0u : tickets[i]);
        if (fill || zero) tickets[i] = q;
    }
    const uint64_t sum = wave_sum(q);
    if (((int)threadIdx.x & 63) == 0) level1[node] = sum;
}

// The write-back: entry i's ticket replaces a nonzero leaf (a zero leaf holds no transition and
// stays); the exchanged old values make the level-1 deltas telescope whatever the order, so level 1
// stays the exact sum under duplicate indices.  The levels above are summed again afterwards.
__global__ void __launch_bounds__(256) per_update_kernel(uint32_t *tickets, uint64_t *level1,
                                                         uint32_t *max_ticket, int S, int E,
                                                         int frac_bits, const int32_t *indices,
                                                         const float *weights, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t q = 0u;
    if (i < B) {
        q = per_ticket(weights[i], frac_bits);
        int s = indices[i], e = indices[(long long)B + i];
        clamp_pair(s, e, S, E);
        const long long leaf = (long long)s * E + e;
        if (tickets[leaf] != 0u) {
            const uint32_t old = atomicExch(&tickets[leaf], q);
            atomicAdd((unsigned long long *)&level1[leaf >> 6],
                      (unsigned long long)((long long)q - (long long)old));
        }
    }
    // one atomicMax per wave
    const uint32_t top = wave_reduce(q, [](uint32_t p, uint32_t o) { return o > p ? o : p; });
    if (((int)threadIdx.x & 63) == 0 && top != 0u) atomicMax(max_ticket, top);
}

// The descent, by a group of G lanes that share one u (< total, or total == 0): at each level the
// group reads the 64 children of its node, 64 / G consecutive ones per lane, forms their inclusive
// prefix sums and counts the children among the first 63 whose prefix is <= u: that count is the
// child holding u, and u continues less the prefix before it.  Children past the end count as 0.
// Tree words are not trusted: the child is at most 63 by construction and every index is clamped
// to its level, so a wrong tree gives a wrong leaf and no address outside tickets / tree.  Returns
// the leaf (the same in every lane of the group); q = its ticket as the tree saw it.
template <int G>
__device__ __forceinline__ long long per_descend(const PerTree &t, uint64_t u, int lane, uint32_t &q)
{
    constexpr int K = 64 / G;
    long long node = 0;
    uint64_t val = 0;
    for (int k = t.levels; k >= 1; --k) {
        const long long n = t.cnt[k - 1];
        const uint64_t *words = t.tree + t.off[k - 1];       // k == 1: not read
        const long long first = node * 64 + (long long)lane * K;
        uint64_t c[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const long long idx = first + i;
            c[i] = idx < n ? (k == 1 ? (uint64_t)t.tickets[idx] : words[idx]) : 0ull;
        }
#pragma unroll
        for (int i = 1; i < K; ++i) c[i] += c[i - 1];
        uint64_t run = c[K - 1];                              // inclusive scan of the lanes' totals
#pragma unroll
        for (int d = 1; d < G; d *= 2) {
            const uint64_t o = (uint64_t)__shfl_up((unsigned long long)run, d, G);
            run += lane >= d ? o : 0ull;
        }
        const uint64_t before = run - c[K - 1];
        int child = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const bool le = before + c[i] <= u && lane * K + i < 63;
            child += __popcll(group_ballot<G>(le));
        }
        uint64_t lo = before, hi = before + c[0];             // of child (child % K) of this lane
#pragma unroll
        for (int i = 1; i < K; ++i) {
            if (i == (child & (K - 1))) {
                lo = before + c[i - 1];
                hi = before + c[i];
            }
        }
        lo = (uint64_t)__shfl((unsigned long long)lo, child / K, G);
        hi = (uint64_t)__shfl((unsigned long long)hi, child / K, G);
        u -= lo;
        val = hi - lo;
        node = node * 64 + child;
        node = node > n - 1 ? n - 1 : node;
    }
    q = (uint32_t)val;
    return node;
}

// u -> the pair of its leaf: 16 lanes per value
__global__ void __launch_bounds__(256) per_find_kernel(const PerTree t, int E, const uint64_t *u_in,
                                                       int B, int32_t *indices_out)
{
    constexpr int G = 16;
    int lane;
    const long long b = group_sample<G>(lane);
    if (b >= B) return;
    const uint64_t total = t.tree[0];
    uint64_t u = u_in[b];
    u = total == 0 ? 0 : (u < total ? u : total - 1);
    uint32_t q;
    long long leaf = per_descend<G>(t, u, lane, q);
    leaf = total == 0 ? 0 : leaf;
    if (lane == 0) {
        int s, e;
        leaf_pair(leaf, E, s, e);
        indices_out[b] = s;
        indices_out[(long long)B + b] = e;
    }
}

// The ticket draw: the uniform draw's Philox words, u = umul64hi(x0:x1, total), the descent -> s, e
// and the probability q / total; head is read only for the age.  Publishes the probability ([B] or
// NULL) and the pair.
struct TicketDraw {
    PerTree t;
    float *probabilities;
    template <int G, bool NSTEP>
    __device__ __forceinline__ Drawn pair(const GatherArgs &a, long long b, int lane) const
    {
        const uint64_t total = t.tree[0];
        uint32_t x0, x1;
        sample_words(a, b, x0, x1);
        const uint64_t u = __umul64hi(((uint64_t)x0 << 32) | x1, total);   // < total, or 0 == total
        uint32_t q;
        long long leaf = per_descend<G>(t, u, lane, q);
        leaf = total == 0 ? 0 : leaf;
        Drawn d = {};
        d.prob = (float)((double)q / (double)total);
        leaf_pair(leaf, a.v.n_envs, d.s, d.e);
        scalar_pair<G>(d);
        if (NSTEP) d.age = steps_behind(a.head[0], d.s, a.v.n_slots);
        if (NSTEP && G == 64) d.age = __builtin_amdgcn_readfirstlane(d.age);
        return d;
    }
    template <bool NSTEP>
    __device__ __forceinline__ void publish(const GatherArgs &a, const Drawn &d, long long b) const
    {
        if (probabilities != nullptr) probabilities[b] = d.prob;
        store_pair(a.indices_out, b, a.o.batch_size, d.s, d.e);
    }
};

// The sampler: one sample per group of G lanes, its pair from the draw source, its rows by the return
// form of Args (GatherArgs: one step, which ends at the newest and needs no age; NStepArgs).  The draw
// publishes with the group's last stores, not ahead of the loads (but see UniformDraw).
// `more`: the draw source where it holds anything -- an empty one is no kernel argument, so the uniform
// and caller forms take the argument bytes they always took.
template <int G, typename V, typename Draw, typename Args, typename... More>
__global__ void __launch_bounds__(256) replay_sample_kernel(const Args args, const More... more)
{
    constexpr bool NSTEP = std::is_same<Args, NStepArgs>::value;
    const Draw draw{more...};
    const GatherArgs &a = args;
    int lane;
    const long long b = group_sample<G>(lane);
    if (b >= a.o.batch_size) return;

    const Drawn d = draw.template pair<G, NSTEP>(a, b, lane);
    const auto last = [&] { draw.template publish<NSTEP>(a, d, b); };
    if constexpr (NSTEP)
        nstep_rows<G, V>(args, b, lane, d.s, d.e, d.age, last);
    else
        gather_rows<G, V>(args, b, lane, d.s, d.e, last);
}

// One launch of the sampler for lane groups of G and 16-byte (vec) or dword units: 256 / G samples per
// block, on the device of the batch.  `more`: the draw source, unless it is empty.
template <typename Draw, typename Args, typename... More>
int launch_sampler(int G, bool vec, const Args &args, void *stream, const More &...more)
{
    const finenv_replay_batch &o = args.o;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(o.observations));
    const auto launch = [&](auto g) {
        constexpr int GG = decltype(g)::value;
        const dim3 grid((unsigned)(((long long)o.batch_size * GG + 255) / 256));
        const auto kernel = vec ? &replay_sample_kernel<GG, f4, Draw, Args, More...>
                                : &replay_sample_kernel<GG, float, Draw, Args, More...>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, args, more...);
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

// 1 <= n_steps <= S - 1 (a window never reaches round to its own start), gamma finite in [0, 1], head
// and discounts present.
bool nstep_ok(const finenv_replay_view &v, const finenv_replay_nstep *ns)
{
    return ns->head && ns->discounts && ns->n_steps >= 1 && ns->n_steps <= v.n_slots - 1 &&
           ns->gamma >= 0.0f && ns->gamma <= 1.0f;
}

// The launch of every sampling call: the gather's checks, those of `ns` where the call is n-step
// (else NULL), then the one kernel with the call's draw source (`more`: as in launch_sampler).
template <typename Draw, typename... More>
int launch_sample(const GatherArgs &a, const finenv_replay_nstep *ns, void *stream, const More &...more)
{
    bool vec = false;
    const int G = gather_group(a.v, a.o, vec);
    if (G == 0 || (ns && !nstep_ok(a.v, ns))) return FINENV_ERR_INVALID;
    if (!ns) return launch_sampler<Draw>(G, vec, a, stream, more...);
    const NStepArgs na = {a, ns->discounts, ns->steps, ns->n_steps, ns->gamma};
    return launch_sampler<Draw>(G, vec, na, stream, more...);
}

// The kernel arguments of a drawn call and of a call with the caller's indices.
GatherArgs drawn_args(const finenv_replay_view *view, const finenv_replay_batch *batch,
                      const int32_t *head, const int64_t *draw, uint64_t seed, int32_t *indices_out)
{
    return {*view, *batch, head, draw, nullptr, indices_out, (uint32_t)seed, (uint32_t)(seed >> 32)};
}

GatherArgs index_args(const finenv_replay_view *view, const finenv_replay_batch *batch,
                      const int32_t *head, const int32_t *indices)
{
    return {*view, *batch, head, nullptr, indices, nullptr, 0u, 0u};
}

// The level table of n leaves (1 <= n <= 2^31 - 1) -> the number of tree words.
long long per_levels(long long n, PerTree &t)
{
    t.cnt[0] = n;
    int k = 0;
    do {
        ++k;
        t.cnt[k] = (t.cnt[k - 1] + 63) / 64;
    } while (t.cnt[k] > 1);
    t.levels = k;
    long long words = 0;
    for (int j = k; j >= 1; --j) {
        t.off[j] = words;
        words += t.cnt[j];
    }
    t.off[0] = 0;                                 // unused: level 0 is the tickets
    for (int j = k + 1; j <= PER_MAX_LEVELS; ++j) t.cnt[j] = t.off[j] = 0;
    return words;
}

// The struct's checks (no HIP call before they pass) and the level table of S x E leaves.
bool per_tree(const finenv_replay_per *per, int32_t S, int32_t E, PerTree &t)
{
    if (!per || !per->tickets || !per->tree || !per->max_ticket || per->frac_bits < 0 ||
        per->frac_bits > 31 || S < 2 || E < 1 || (long long)S * E > 0x7fffffffLL)
        return false;
    t.tickets = per->tickets;
    t.tree = per->tree;
    per_levels((long long)S * E, t);
    return true;
}

// Levels `from` .. the root, each from the one below it: one launch per level.
int per_sum_levels(const PerTree &t, int from, void *stream)
{
    for (int k = from; k <= t.levels; ++k) {
        const dim3 grid((unsigned)((t.cnt[k] + 3) / 4));
        if (k == 1)
            hipLaunchKernelGGL(per_sum_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)stream,
                               (const uint32_t *)t.tickets, t.cnt[0], t.tree + t.off[1], t.cnt[1]);
        else
            hipLaunchKernelGGL(per_sum_kernel<uint64_t>, grid, dim3(256), 0, (hipStream_t)stream,
                               (const uint64_t *)(t.tree + t.off[k - 1]), t.cnt[k - 1],
                               t.tree + t.off[k], t.cnt[k]);
    }
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
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
    const GatherArgs a = drawn_args(view, batch, head, draw, seed, indices_out);
    return launch_sample<UniformDraw>(a, nullptr, stream);
}

extern "C" int finenv_replay_gather(const finenv_replay_view *view, const int32_t *indices,
                                    const finenv_replay_batch *batch, void *stream)
{
    if (!view || !batch || !indices) return FINENV_ERR_INVALID;
    return launch_sample<CallerDraw>(index_args(view, batch, nullptr, indices), nullptr, stream);
}

extern "C" int finenv_replay_sample_nstep(const finenv_replay_view *view, const int32_t *head,
                                          const int64_t *draw, uint64_t seed,
                                          const finenv_replay_batch *batch,
                                          const finenv_replay_nstep *nstep, int32_t *indices_out,
                                          void *stream)
{
    if (!view || !batch || !head || !draw || !nstep) return FINENV_ERR_INVALID;
    const GatherArgs a = drawn_args(view, batch, head, draw, seed, indices_out);
    return launch_sample<UniformDraw>(a, nstep, stream);
}

extern "C" int finenv_replay_gather_nstep(const finenv_replay_view *view, const int32_t *indices,
                                          const finenv_replay_batch *batch,
                                          const finenv_replay_nstep *nstep, void *stream)
{
    if (!view || !batch || !indices || !nstep) return FINENV_ERR_INVALID;
    return launch_sample<CallerDraw>(index_args(view, batch, nstep->head, indices), nstep, stream);
}

extern "C" int64_t finenv_replay_per_tree_words(int64_t n_leaves)
{
    if (n_leaves < 1 || n_leaves > 0x7fffffffLL) return -1;
    PerTree t;
    return per_levels(n_leaves, t);
}

extern "C" int finenv_replay_per_rebuild(const finenv_replay_per *per, int32_t n_slots, int32_t n_envs,
                                         void *stream)
{
    PerTree t;
    if (!per_tree(per, n_slots, n_envs, t)) return FINENV_ERR_INVALID;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(per->tree));
    return per_sum_levels(t, 1, stream);
}

extern "C" int finenv_replay_per_put(const finenv_replay_per *per, int32_t n_slots, int32_t n_envs,
                                     int32_t pos, int32_t pos_next, void *stream)
{
    PerTree t;
    if (!per_tree(per, n_slots, n_envs, t) || pos < 0 || pos >= n_slots || pos_next < 0 ||
        pos_next >= n_slots)
        return FINENV_ERR_INVALID;
    const long long E = n_envs;
    const long long fill0 = pos * E, fill1 = fill0 + E;
    const long long zero0 = pos_next * E, zero1 = pos_next == pos ? zero0 : zero0 + E;
    // the level-1 nodes over the two runs of leaves; runs whose nodes meet become one
    long long a0 = fill0 >> 6, a1 = (fill1 - 1) >> 6, b0 = 0, nb = 0;
    if (zero1 > zero0) {
        const long long z0 = zero0 >> 6, z1 = (zero1 - 1) >> 6;
        if (z0 <= a1 && a0 <= z1) {
            a0 = z0 < a0 ? z0 : a0;
            a1 = z1 > a1 ? z1 : a1;
        } else {
            b0 = z0;
            nb = z1 - z0 + 1;
        }
    }
    const long long na = a1 - a0 + 1;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(per->tree));
    hipLaunchKernelGGL(per_put_kernel, dim3((unsigned)((na + nb + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, t.tickets, t.tree + t.off[1], t.cnt[0],
                       (const uint32_t *)per->max_ticket, fill0, fill1, zero0, zero1, a0, na, b0, nb);
    return per_sum_levels(t, 2, stream);
}

extern "C" int finenv_replay_per_update(const finenv_replay_per *per, int32_t n_slots, int32_t n_envs,
                                        const int32_t *indices, const float *weights,
                                        int32_t batch_size, void *stream)
{
    PerTree t;
    if (!per_tree(per, n_slots, n_envs, t) || !indices || !weights || batch_size < 1)
        return FINENV_ERR_INVALID;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(per->tree));
    hipLaunchKernelGGL(per_update_kernel, dim3((unsigned)(((long long)batch_size + 255) / 256)),
                       dim3(256), 0, (hipStream_t)stream, t.tickets, t.tree + t.off[1], per->max_ticket,
                       n_slots, n_envs, per->frac_bits, indices, weights, batch_size);
    return per_sum_levels(t, 2, stream);
}

extern "C" int finenv_replay_per_find(const finenv_replay_per *per, int32_t n_slots, int32_t n_envs,
                                      const uint64_t *u, int32_t batch_size, int32_t *indices_out,
                                      void *stream)
{
    PerTree t;
    if (!per_tree(per, n_slots, n_envs, t) || !u || !indices_out || batch_size < 1)
        return FINENV_ERR_INVALID;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(per->tree));
    hipLaunchKernelGGL(per_find_kernel, dim3((unsigned)(((long long)batch_size + 15) / 16)), dim3(256),
                       0, (hipStream_t)stream, t, n_envs, u, batch_size, indices_out);
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
}

extern "C" int finenv_replay_per_sample(const finenv_replay_view *view, const finenv_replay_per *per,
                                        const int64_t *draw, uint64_t seed,
                                        const finenv_replay_batch *batch, float *probabilities_out,
                                        int32_t *indices_out, void *stream)
{
    TicketDraw d = {{}, probabilities_out};
    if (!view || !batch || !draw || !per_tree(per, view->n_slots, view->n_envs, d.t))
        return FINENV_ERR_INVALID;
    const GatherArgs a = drawn_args(view, batch, nullptr, draw, seed, indices_out);
    return launch_sample<TicketDraw>(a, nullptr, stream, d);
}

extern "C" int finenv_replay_per_sample_nstep(const finenv_replay_view *view,
                                              const finenv_replay_per *per, const int64_t *draw,
                                              uint64_t seed, const finenv_replay_batch *batch,
                                              const finenv_replay_nstep *nstep, float *probabilities_out,
                                              int32_t *indices_out, void *stream)
{
    TicketDraw d = {{}, probabilities_out};
    if (!view || !batch || !draw || !nstep || !per_tree(per, view->n_slots, view->n_envs, d.t))
        return FINENV_ERR_INVALID;
    const GatherArgs a = drawn_args(view, batch, nstep->head, draw, seed, indices_out);
    return launch_sample<TicketDraw>(a, nstep, stream, d);
}
