// finenv_vecnorm.hip -- running observation / return statistics (SB3's VecNormalize / RunningMeanStd,
// contract in include/finenv.h) over [n_rows][dim] float32 with a row pitch (gfx950).
// Moments: ONE read of the batch.  Lanes own columns (a 16-byte unit or a dword each, the rule of
// finenv_rollout_minibatch), G unit-lanes side by side and 1024 / G row-lanes above each other, so a
// wave reads 64 / G whole row segments of 256 bytes.  A block owns one column chunk of one row tile;
// every lane of the block shifts by the SAME K, the tile's first row, so the lanes' float64 sums of
// (x - K) and (x - K)^2 merge by plain addition in a fixed order (xor-shuffles inside the wave, then
// the 16 waves through LDS), and one (mean, M2) per tile and column goes to the partials buffer.  The
// block that takes the last ticket merges the tiles by Chan's rule in a fixed order and then the batch
// into the running stats; nobody waits for anybody, no floating-point atomic exists, and the order
// depends on (n_rows, dim, unit size) only, so a call repeats bit for bit.  At most
// FINENV_VECNORM_MAX_TILES tiles: the partials buffer has a fixed size and the last block's serial
// merge stays short.
// Apply: elementwise, the same lane layout in 256-thread blocks; mean and scale are loaded once per
// lane, four rows are loaded before the first of them is stored (a load behind the wave's own stores
// waits for them), and each lane writes exactly the columns it read, so out == x works.
// The return column, the reward normalisation and the done handling of a VecNormalize step are extra
// blocks of the same two launches.  Every offset is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finenv.h"
#include "finenv_host.h"
#include "finenv_group.h"       // f4

namespace {

constexpr int MB = 1024;                          // threads of a moments block
constexpr int MW = MB / 64;                       // its waves
constexpr int AB = 256;                           // threads of an apply block
constexpr int APPLY_ROWS = 16;                    // rows per lane of an apply block
constexpr int MAX_TILES = FINENV_VECNORM_MAX_TILES;
static_assert(MAX_TILES <= MB && 2 * MB <= MW * 64 * 2, "the last block's merge reuses the reduction block");

struct Stats {                                    // what the kernels need of a finenv_vecnorm
    double *mean, *var, *scale, *count, *partials;
    double epsilon;
    int dim;
};

struct MatJob {                                   // the float32 matrix of a moments launch
    const float *x;
    long long n_rows, pitch, tile_rows;
    int dim, lg, chunks, tiles;                   // lg = log2 G; chunks of G units; row tiles
};

struct RetJob {                                   // the return column of a training step
    const float *reward;
    double *returns;
    double gamma;
    long long n, tile_rows;
    int tiles;
};

struct MomentsArgs {
    Stats a, b;                                   // of the matrix / of the return column
    MatJob m;
    RetJob r;
    int blocks_a;                                 // m.chunks * m.tiles matrix blocks, then r.tiles blocks
    uint32_t total;
    uint32_t *ticket;
};

struct ApplyArgs {
    const float *x;
    float *out;
    long long n_rows, pitch_in, pitch_out, tile_rows;
    const double *mean, *scale;
    double clip;
    int dim, lg, chunks, mode;                    // mode 0: copy, 1: scale and clip, 2: centre too
    int blocks_a;                                 // matrix blocks, then the reward blocks
    const float *reward;                          // the reward part of a step (n_envs 0: none)
    float *reward_out;
    const uint8_t *done;
    uint8_t *done_out;                            // or NULL
    double *returns;
    const double *ret_scale;
    double ret_clip;
    int n_envs, reward_mode, zero_returns;        // reward_mode 0: copy, 1: scale and clip
};

template <typename V>
__device__ __forceinline__ float comp(const V &v, int c)
{
    if constexpr (sizeof(V) == sizeof(float)) return v;
    else return v[c];
}

template <typename V>
__device__ __forceinline__ void set_comp(V &v, int c, float x)
{
    if constexpr (sizeof(V) == sizeof(float)) v = x;
    else v[c] = x;
}

// The unit at p: whole, or (f4 only) the `left` < 4 columns the row still has -- the pad is never read.
template <typename V>
__device__ __forceinline__ V load_unit(const float *p, long long left, bool full)
{
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    if (full) return *(const V *)p;
    V v = {};
#pragma unroll
    for (int c = 0; c < VW; ++c)
        if (c < left) set_comp(v, c, p[c]);
    return v;
}

template <typename V>
__device__ __forceinline__ void store_unit(float *p, const V &v, long long left, bool full)
{
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    if (full) {
        *(V *)p = v;
        return;
    }
#pragma unroll
    for (int c = 0; c < VW; ++c)
        if (c < left) p[c] = comp(v, c);
}

// The block's sums of one tile -> (mean, M2) per column in the partials buffer.  Every lane holds the
// sums of its VW columns over its rows, all shifted by the tile's K.  Lanes 64 / G apart in a wave
// hold the same columns: xor-shuffles add them (both partners form the same sum); then lanes < G of
// every wave park theirs in LDS and lane j < G * VW of the block adds the 16 waves' in wave order.
template <int VW>
__device__ __forceinline__ void tile_store(double (&s1)[VW], double (&s2)[VW], const double (&K)[VW],
                                           int lg, double *partials, int tile, double n_t,
                                           long long col0, int dim, double *red, double *ks)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, G = 1 << lg, ul = lane & (G - 1);
    for (int o = G; o < 64; o <<= 1) {
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            s1[c] += __shfl_xor(s1[c], o);
            s2[c] += __shfl_xor(s2[c], o);
        }
    }
    if (lane < G) {
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            red[(w * 64 + ul * VW + c) * 2] = s1[c];
            red[(w * 64 + ul * VW + c) * 2 + 1] = s2[c];
            if (w == 0) ks[ul * VW + c] = K[c];
        }
    }
    __syncthreads();
    if (tid < G * VW) {
        const long long col = col0 + tid;
        if (col < dim) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < MW; ++k) {
                a += red[(k * 64 + tid) * 2];
                b += red[(k * 64 + tid) * 2 + 1];
            }
            const double m = a / n_t;
            const double m2 = b - a * m;                       // sum (x-K)^2 - (sum (x-K))^2 / n
            // write-through (agent-scope) stores: another block reads them in this launch, and a
            // release fence per block would write the whole L2 back
            __hip_atomic_store(partials + (long long)tile * 2 * dim + col, ks[tid] + m, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(partials + ((long long)tile * 2 + 1) * dim + col, m2 < 0.0 ? 0.0 : m2,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);               // (a NaN stays)
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // drained before the block's ticket
    }
}

template <typename V>
__device__ __forceinline__ void matrix_tile(const MatJob &m, int b, double *partials, double *red,
                                            double *ks)
{
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    const int tid = (int)threadIdx.x, G = 1 << m.lg, ul = tid & (G - 1);
    const int rl = tid >> m.lg, RL = MB >> m.lg;
    const int chunk = b % m.chunks, tile = b / m.chunks;
    const long long col0 = ((long long)chunk * G + ul) * VW, left = m.dim - col0;
    const bool active = left > 0, full = left >= VW;
    const long long t0 = (long long)tile * m.tile_rows;
    const long long t1 = t0 + m.tile_rows < m.n_rows ? t0 + m.tile_rows : m.n_rows;
    double K[VW], s1[VW], s2[VW];
#pragma unroll
    for (int c = 0; c < VW; ++c) K[c] = s1[c] = s2[c] = 0.0;
    if (active) {
        const float *base = m.x + col0;
        const V kv = load_unit<V>(base + t0 * m.pitch, left, full);
#pragma unroll
        for (int c = 0; c < VW; ++c) K[c] = (double)comp(kv, c);
        for (long long r = t0 + rl; r < t1; r += 4ll * RL) {
            V x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                      // a row past the tile counts as K: adds 0
                const long long rr = r + (long long)j * RL;
                x[j] = kv;
                if (rr < t1) x[j] = load_unit<V>(base + rr * m.pitch, left, full);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int c = 0; c < VW; ++c) {
                    const double d = (double)comp(x[j], c) - K[c];
                    s1[c] += d;
                    s2[c] += d * d;
                }
            }
        }
    }
    tile_store<VW>(s1, s2, K, m.lg, partials, tile, (double)(t1 - t0), (long long)chunk * G * VW, m.dim,
                   red, ks);
}

// returns[e] = returns[e] * gamma + reward[e] over one tile of envs, and the tile's moments of the
// new values.  K is the tile's first new value; every lane reads its inputs before anyone stores.
__device__ __forceinline__ void return_tile(const RetJob &r, int tile, double *partials, double *red,
                                            double *ks)
{
    const int tid = (int)threadIdx.x;
    const long long t0 = (long long)tile * r.tile_rows;
    const long long t1 = t0 + r.tile_rows < r.n ? t0 + r.tile_rows : r.n;
    double K[1], s1[1] = {0.0}, s2[1] = {0.0};
    K[0] = r.returns[t0] * r.gamma + (double)r.reward[t0];
    __syncthreads();
    for (long long e = t0 + tid; e < t1; e += MB) {
        const double x = r.returns[e] * r.gamma + (double)r.reward[e];
        r.returns[e] = x;
        const double d = x - K[0];
        s1[0] += d;
        s2[0] += d * d;
    }
    tile_store<1>(s1, s2, K, 0, partials, tile, (double)(t1 - t0), 0, 1, red, ks);
}

__device__ __forceinline__ double scale_of(double var, double epsilon) { return 1.0 / sqrt(var + epsilon); }

// The last block: the tiles of every column by Chan's rule, then the batch into the running stats
// (include/finenv.h).  The partials were stored write-through and are no longer in L2, so what the
// merge costs is its dependent round trips to memory: up to FIN_GROUPS lanes share a column, each merges
// a run of consecutive tiles with FIN_DEPTH tiles in flight (agent-scope loads behind the block's
// acquire), and lane 0 of the column merges the runs in order through LDS (`grp`).  The order depends
// on (tiles, dim) only.  Inside a run the weights of merging the k-th full tile, h / (k h + h) and
// k h * h / (k h + h), are the same for every column: `wts`, made once, so a merge is five flops.
constexpr int FIN_GROUPS = 16, FIN_DEPTH = 16;

__device__ __forceinline__ void finalize(const Stats &s, int tiles, long long tile_rows, long long n_rows,
                                         double *grp, double *wts)
{
    const int tid = (int)threadIdx.x;
    const double cnt = *s.count;
    if (tid < MAX_TILES) {
        const double h = (double)tile_rows, n = (double)tid * h;
        wts[tid] = h / (n + h);
        wts[MAX_TILES + tid] = n * h / (n + h);
    }
    int S = s.dim <= MB ? MB / s.dim : 1;
    S = S < FIN_GROUPS ? S : FIN_GROUPS;
    const int per = (tiles + S - 1) / S;                      // tiles per run
    S = (tiles + per - 1) / per;                              // no empty run
    const long long run_rows = (long long)per * tile_rows;
    for (int cb = 0; cb < s.dim; cb += MB) {
        const int cw = s.dim - cb < MB ? s.dim - cb : MB;
        const int g = tid / cw, c = cb + tid % cw;
        __syncthreads();                                      // the weights; `grp` free again
        if (g < S) {
            const int ta = g * per, tb = ta + per < tiles ? ta + per : tiles;
            double mean = 0.0, m2 = 0.0;
            for (int t0 = ta; t0 < tb; t0 += FIN_DEPTH) {
                double mb[FIN_DEPTH], qb[FIN_DEPTH];
#pragma unroll
                for (int j = 0; j < FIN_DEPTH; ++j) {         // (past the run: its last tile again, unused)
                    const long long t = t0 + j < tb ? t0 + j : tb - 1;
                    mb[j] = __hip_atomic_load(s.partials + t * 2 * s.dim + c, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
                    qb[j] = __hip_atomic_load(s.partials + (t * 2 + 1) * s.dim + c, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
                }
#pragma unroll
                for (int j = 0; j < FIN_DEPTH; ++j) {
                    const int t = t0 + j, k = t - ta;
                    if (t >= tb) break;
                    if (k == 0) {
                        mean = mb[j];
                        m2 = qb[j];
                        continue;
                    }
                    double w1 = wts[k], w2 = wts[MAX_TILES + k];
                    if (t == tiles - 1) {                     // the one tile that may be ragged
                        const double n = (double)((long long)k * tile_rows);
                        const double nb = (double)(n_rows - (long long)t * tile_rows);
                        w1 = nb / (n + nb);
                        w2 = n * nb / (n + nb);
                    }
                    const double delta = mb[j] - mean;
                    mean += delta * w1;
                    m2 += qb[j] + delta * delta * w2;
                }
            }
            grp[2 * tid] = mean;
            grp[2 * tid + 1] = m2;
        }
        __syncthreads();
        if (tid < cw) {                                       // lane 0 of the column: the runs in order
            double mean = grp[2 * tid], m2 = grp[2 * tid + 1];
            double n = (double)(run_rows < n_rows ? run_rows : n_rows);
            for (int r = 1; r < S; ++r) {
                const long long left = n_rows - r * run_rows;
                const double nb = (double)(left < run_rows ? left : run_rows), tot = n + nb;
                const double delta = grp[2 * (r * cw + tid)] - mean;
                mean += delta * nb / tot;
                m2 += grp[2 * (r * cw + tid) + 1] + delta * delta * n * nb / tot;
                n = tot;
            }
            const double bv = m2 / n;
            const double m0 = s.mean[c], v0 = s.var[c];
            const double delta = mean - m0, tot = cnt + n;
            const double v = (v0 * cnt + bv * n + delta * delta * cnt * n / tot) / tot;
            s.mean[c] = m0 + delta * n / tot;
            s.var[c] = v;
            s.scale[c] = scale_of(v, s.epsilon);
        }
    }
    __syncthreads();                              // every lane has read the count
    if (tid == 0) *s.count = cnt + (double)n_rows;
}

template <typename V>
__global__ void __launch_bounds__(MB) vecnorm_moments_kernel(const MomentsArgs a)
{
    __shared__ double red[MW * 64 * 2];
    __shared__ double ks[64];
    __shared__ double wts[2 * MAX_TILES];
    __shared__ int last;
    const int b = (int)blockIdx.x;
    if (b < a.blocks_a)
        matrix_tile<V>(a.m, b, a.a.partials, red, ks);
    else
        return_tile(a.r, b - a.blocks_a, a.b.partials, red, ks);
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(a.ticket, 1u) == a.total - 1u;
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (a.blocks_a) finalize(a.a, a.m.tiles, a.m.tile_rows, a.m.n_rows, red, wts);
    if (a.r.tiles) finalize(a.b, a.r.tiles, a.r.tile_rows, a.r.n, red, wts);
    if (threadIdx.x == 0) atomicExch(a.ticket, 0u);           // a replay starts clean
}

__device__ __forceinline__ float normalise(float x, double mu, double sc, double clip, bool centre)
{
    double y = (double)x;
    if (centre) y = y - mu;
    y = y * sc;
    y = y < -clip ? -clip : y > clip ? clip : y;
    return (float)y;
}

template <typename V>
__global__ void __launch_bounds__(AB) vecnorm_apply_kernel(const ApplyArgs a)
{
    constexpr int VW = (int)(sizeof(V) / sizeof(float));
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    if (b >= a.blocks_a) {                        // the reward part of a step: one env per lane
        const long long e = (long long)(b - a.blocks_a) * AB + tid;
        if (e >= a.n_envs) return;
        const float r = a.reward[e];
        const uint8_t d = a.done[e];
        a.reward_out[e] = a.reward_mode ? normalise(r, 0.0, *a.ret_scale, a.ret_clip, false) : r;
        if (a.zero_returns && d) a.returns[e] = 0.0;
        if (a.done_out != nullptr) a.done_out[e] = d;
        return;
    }
    const int G = 1 << a.lg, ul = tid & (G - 1), rl = tid >> a.lg, RL = AB >> a.lg;
    const int chunk = b % a.chunks, tile = b / a.chunks;
    const long long col0 = ((long long)chunk * G + ul) * VW, left = a.dim - col0;
    if (left <= 0) return;
    const bool full = left >= VW, centre = a.mode == 2;
    double mu[VW], sc[VW];
#pragma unroll
    for (int c = 0; c < VW; ++c) {
        const bool ok = c < left;
        mu[c] = centre && ok ? a.mean[col0 + c] : 0.0;
        sc[c] = a.mode && ok ? a.scale[col0 + c] : 1.0;
    }
    const long long t0 = (long long)tile * a.tile_rows;
    const long long t1 = t0 + a.tile_rows < a.n_rows ? t0 + a.tile_rows : a.n_rows;
    const float *src = a.x + col0;
    float *dst = a.out + col0;
    for (long long r = t0 + rl; r < t1; r += 4ll * RL) {
        V x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long rr = r + (long long)j * RL;
            x[j] = V{};
            if (rr < t1) x[j] = load_unit<V>(src + rr * a.pitch_in, left, full);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long rr = r + (long long)j * RL;
            if (rr >= t1) break;
            V y = x[j];
            if (a.mode) {
#pragma unroll
                for (int c = 0; c < VW; ++c) set_comp(y, c, normalise(comp(x[j], c), mu[c], sc[c], a.clip, centre));
            }
            store_unit<V>(dst + rr * a.pitch_out, y, left, full);
        }
    }
}

__global__ void __launch_bounds__(AB) vecnorm_refresh_kernel(const double *var, double *scale, int dim,
                                                             double epsilon)
{
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c < dim) scale[c] = scale_of(var[c], epsilon);
}

// ---------------------------------------------------------------------------------- host
bool stats_ok(const finenv_vecnorm *s)
{
    return s && s->mean && s->var && s->scale && s->count && s->partials && s->ticket && s->dim >= 1;
}

Stats stats_of(const finenv_vecnorm &s)
{
    return {s.mean, s.var, s.scale, s.count, s.partials, s.epsilon, s.dim};
}

// The lane layout of a [.][dim] matrix: 16-byte units where every base and pitch allows it, G
// unit-lanes (a power of two, at most 256 bytes of a row) and the column chunks of G units.
struct Layout {
    bool vec;
    int lg, chunks;
};

Layout layout_for(int dim, uintptr_t bases, long long pitches)
{
    Layout l;
    l.vec = (bases & 15) == 0 && (pitches & 3) == 0 && dim >= 4;
    const int units = l.vec ? (dim + 3) / 4 : dim, cap = l.vec ? 16 : 64;
    l.lg = 0;
    while ((1 << l.lg) < cap && (1 << l.lg) < units) ++l.lg;
    l.chunks = (units + (1 << l.lg) - 1) >> l.lg;
    return l;
}

// n rows in at most MAX_TILES tiles whose height is a multiple of the `rl` row-lanes of a block
void tiles_for(long long n, int rl, long long &tile_rows, int &tiles)
{
    const long long per = (long long)rl * MAX_TILES;
    tile_rows = (n + per - 1) / per * rl;
    tiles = (int)((n + tile_rows - 1) / tile_rows);
}

// The moments launch of a matrix (stats != NULL) and / or a return column (ret != NULL), one ticket.
// FINENV_ERR_INVALID when a partials buffer is too small or the grid too large.
int launch_moments(const finenv_vecnorm *stats, const float *x, long long n_rows, long long pitch,
                   const finenv_vecnorm *ret, const float *reward, double *returns, double gamma,
                   long long n_envs, hipStream_t stream)
{
    MomentsArgs a = {};
    bool vec = false;
    if (stats) {
        const Layout l = layout_for(stats->dim, (uintptr_t)x, pitch);
        vec = l.vec;
        a.a = stats_of(*stats);
        a.m.x = x;
        a.m.n_rows = n_rows;
        a.m.pitch = pitch;
        a.m.dim = stats->dim;
        a.m.lg = l.lg;
        a.m.chunks = l.chunks;
        tiles_for(n_rows, MB >> l.lg, a.m.tile_rows, a.m.tiles);
        if (2ll * a.m.tiles * stats->dim > stats->partials_cap) return FINENV_ERR_INVALID;
        if ((long long)a.m.chunks * a.m.tiles > 0x3fffffffll) return FINENV_ERR_INVALID;
        a.blocks_a = a.m.chunks * a.m.tiles;
    }
    if (ret) {
        a.b = stats_of(*ret);
        a.r.reward = reward;
        a.r.returns = returns;
        a.r.gamma = gamma;
        a.r.n = n_envs;
        tiles_for(n_envs, MB, a.r.tile_rows, a.r.tiles);
        if (2ll * a.r.tiles > ret->partials_cap) return FINENV_ERR_INVALID;
    }
    a.total = (uint32_t)(a.blocks_a + a.r.tiles);
    a.ticket = stats ? stats->ticket : ret->ticket;
    const auto kernel = vec ? &vecnorm_moments_kernel<f4> : &vecnorm_moments_kernel<float>;
    hipLaunchKernelGGL(kernel, dim3(a.total), dim3(MB), 0, stream, a);
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
}

// The matrix part of an apply launch (mode: ApplyArgs); false when the grid would be too large.
bool apply_matrix(ApplyArgs &a, bool &vec, const finenv_vecnorm &s, const float *x, long long n_rows,
                  long long pitch_in, float *out, long long pitch_out, int mode)
{
    const Layout l = layout_for(s.dim, (uintptr_t)x | (uintptr_t)out, pitch_in | pitch_out);
    vec = l.vec;
    a.x = x;
    a.out = out;
    a.n_rows = n_rows;
    a.pitch_in = pitch_in;
    a.pitch_out = pitch_out;
    a.tile_rows = (long long)(AB >> l.lg) * APPLY_ROWS;
    a.mean = s.mean;
    a.scale = s.scale;
    a.clip = s.clip;
    a.dim = s.dim;
    a.lg = l.lg;
    a.chunks = l.chunks;
    a.mode = mode;
    const long long blocks = (n_rows + a.tile_rows - 1) / a.tile_rows * l.chunks;
    if (blocks > 0x3fffffffll) return false;
    a.blocks_a = (int)blocks;
    return true;
}

int launch_apply(const ApplyArgs &a, bool vec, hipStream_t stream)
{
    const unsigned grid = (unsigned)a.blocks_a + (unsigned)((a.n_envs + AB - 1) / AB);
    const auto kernel = vec ? &vecnorm_apply_kernel<f4> : &vecnorm_apply_kernel<float>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(AB), 0, stream, a);
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
}
}  // namespace

extern "C" int finenv_vecnorm_refresh(const finenv_vecnorm *stats, void *stream)
{
    if (!stats_ok(stats)) return FINENV_ERR_INVALID;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(stats->mean));
    hipLaunchKernelGGL(vecnorm_refresh_kernel, dim3((stats->dim + AB - 1) / AB), dim3(AB), 0,
                       (hipStream_t)stream, stats->var, stats->scale, stats->dim, stats->epsilon);
    return hipGetLastError() == hipSuccess ? FINENV_OK : FINENV_ERR_HIP;
}

extern "C" int finenv_vecnorm_update(const finenv_vecnorm *stats, const float *x, int64_t n_rows,
                                     int64_t pitch, void *stream)
{
    if (!stats_ok(stats) || !x || n_rows < 1 || pitch < stats->dim) return FINENV_ERR_INVALID;
    // the refusals of launch_moments, before the device is touched
    {
        const Layout l = layout_for(stats->dim, (uintptr_t)x, pitch);
        long long tile_rows;
        int tiles;
        tiles_for(n_rows, MB >> l.lg, tile_rows, tiles);
        if (2ll * tiles * stats->dim > stats->partials_cap) return FINENV_ERR_INVALID;
    }
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(stats->mean));
    return launch_moments(stats, x, n_rows, pitch, nullptr, nullptr, nullptr, 0.0, 0, (hipStream_t)stream);
}

extern "C" int finenv_vecnorm_apply(const finenv_vecnorm *stats, const float *x, int64_t n_rows,
                                    int64_t pitch_in, float *out, int64_t pitch_out, int32_t center,
                                    void *stream)
{
    if (!stats_ok(stats) || !x || !out || n_rows < 1 || pitch_in < stats->dim || pitch_out < stats->dim)
        return FINENV_ERR_INVALID;
    ApplyArgs a = {};
    bool vec;
    if (!apply_matrix(a, vec, *stats, x, n_rows, pitch_in, out, pitch_out, center ? 2 : 1))
        return FINENV_ERR_INVALID;
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(out));
    return launch_apply(a, vec, (hipStream_t)stream);
}

extern "C" int finenv_vecnorm_step(const finenv_vecnorm *obs_stats, const finenv_vecnorm *ret_stats,
                                   const float *obs, int64_t obs_pitch, const float *reward,
                                   const uint8_t *done, double *returns, double gamma, float *obs_out,
                                   int64_t obs_out_pitch, float *reward_out, uint8_t *done_out,
                                   int32_t n_envs, int32_t training, int32_t norm_obs,
                                   int32_t norm_reward, void *stream)
{
    if (!stats_ok(obs_stats) || !stats_ok(ret_stats) || ret_stats->dim != 1 || !obs || !reward || !done ||
        !returns || !obs_out || !reward_out || n_envs < 1 || obs_pitch < obs_stats->dim ||
        obs_out_pitch < obs_stats->dim)
        return FINENV_ERR_INVALID;
    ApplyArgs a = {};
    bool vec;
    if (!apply_matrix(a, vec, *obs_stats, obs, n_envs, obs_pitch, obs_out, obs_out_pitch, norm_obs ? 2 : 0))
        return FINENV_ERR_INVALID;
    a.reward = reward;
    a.reward_out = reward_out;
    a.done = done;
    a.done_out = done_out;
    a.returns = returns;
    a.ret_scale = ret_stats->scale;
    a.ret_clip = ret_stats->clip;
    a.n_envs = n_envs;
    a.reward_mode = norm_reward ? 1 : 0;
    a.zero_returns = training && norm_reward;
    const bool upd_obs = training && norm_obs, upd_ret = training && norm_reward;
    if (upd_obs || upd_ret) {                     // the refusals of launch_moments, before any launch
        long long tile_rows;
        int tiles;
        if (upd_obs) {
            const Layout l = layout_for(obs_stats->dim, (uintptr_t)obs, obs_pitch);
            tiles_for(n_envs, MB >> l.lg, tile_rows, tiles);
            if (2ll * tiles * obs_stats->dim > obs_stats->partials_cap) return FINENV_ERR_INVALID;
        }
        if (upd_ret) {
            tiles_for(n_envs, MB, tile_rows, tiles);
            if (2ll * tiles > ret_stats->partials_cap) return FINENV_ERR_INVALID;
        }
    }
    const finenv_host::DeviceGuard guard(finenv_host::pointer_device(obs_out));
    if (upd_obs || upd_ret) {
        const int rc = launch_moments(upd_obs ? obs_stats : nullptr, obs, n_envs, obs_pitch,
                                      upd_ret ? ret_stats : nullptr, reward, returns, gamma, n_envs,
                                      (hipStream_t)stream);
        if (rc) return rc;
    }
    return launch_apply(a, vec, (hipStream_t)stream);
}
