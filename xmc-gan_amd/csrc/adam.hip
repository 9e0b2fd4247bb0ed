// Multi-tensor Adam: one launch updates every parameter tensor of a network
// (torch.optim.Adam.step at train_gan.py:229,252,289: eps 1e-8, no weight decay, no amsgrad).
// The table lives in device memory and is static while the parameter/gradient storage is, so the
// launch is hipGraph-capturable; per-tensor step counters are kept on the device as well.
// Second half of the file: the exponential moving average of the weights, on its own and fused into the Adam update.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int CHUNK = NT * 4 * 4;  // elements per block: 4 float4 per thread

// Dynamic loss scale (the IEEE-half mode; torch.cuda.amp.GradScaler's rule, device-resident so the step stays capturable):
//   sf[0] = scale, sf[1] = 1 / scale;  si[0] = a gradient of THIS step was not finite, si[1] = consecutive finite steps,
//   si[2] = si[0] of the last finished step, si[3] = steps skipped so far.
// adam_check_kernel raises si[0]; adam_kernel and adam_bump_kernel leave parameters, moments and step counters alone when it
// is set; scaler_update_kernel backs the scale off (or grows it after `interval` finite steps) and clears the flag.
__global__ void adam_check_kernel(const XmcAdamEntry* __restrict__ tab, const int2* __restrict__ chunks, int* __restrict__ si) {
    const int2 c = chunks[blockIdx.x];
    const XmcAdamEntry e = tab[c.x];
    const int64_t base = (int64_t)c.y * CHUNK;
    const int64_t lim = e.n - base < CHUNK ? e.n - base : CHUNK;
    const float* g = e.grad + base;
    bool bad = false;
    // |x| < inf is false for inf and NaN alike
    if ((e.n & 3) == 0) {
        for (int i = threadIdx.x * 4; i < lim; i += NT * 4) {
            const f32x4 G = *reinterpret_cast<const f32x4*>(g + i);
            bad |= !(fabsf(G[0]) < INFINITY) | !(fabsf(G[1]) < INFINITY) | !(fabsf(G[2]) < INFINITY) | !(fabsf(G[3]) < INFINITY);
        }
    } else {
        for (int i = threadIdx.x; i < lim; i += NT) bad |= !(fabsf(g[i]) < INFINITY);
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(si, 1);
}
__global__ void scaler_update_kernel(float* __restrict__ sf, int* __restrict__ si, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float sc = sf[0];
    const int bad = si[0];
    if (bad) {
        sc = fmaxf(sc * backoff, 1.f);
        si[1] = 0;
        si[3] += 1;
    } else if (++si[1] >= interval) {
        sc = fminf(sc * growth, 16777216.f);
        si[1] = 0;
    }
    sf[0] = sc;
    sf[1] = 1.f / sc;
    si[2] = bad;
    si[0] = 0;
}

__global__ void adam_kernel(const XmcAdamEntry* __restrict__ tab, const int2* __restrict__ chunks,
                            float lr, float b1, float b2, float eps, float gs, const float* __restrict__ sf,
                            const int* __restrict__ si) {
    if (si && *si) return;                      // a non-finite gradient: the whole step is skipped
    if (sf) gs *= sf[1];
    const int2 c = chunks[blockIdx.x];
    const XmcAdamEntry e = tab[c.x];
    const int t = *e.step + 1;
    const float bc1 = 1.f - powf(b1, (float)t), bc2s = sqrtf(1.f - powf(b2, (float)t));
    const float step_size = lr / bc1;
    const int64_t base = (int64_t)c.y * CHUNK;
    const int64_t lim = e.n - base < CHUNK ? e.n - base : CHUNK;
    float* p = e.param + base; const float* g = e.grad + base; float* m = e.m + base; float* v = e.v + base;
    if ((e.n & 3) == 0) {
        for (int i = threadIdx.x * 4; i < lim; i += NT * 4) {
            f32x4 P = *reinterpret_cast<f32x4*>(p + i), G = *reinterpret_cast<const f32x4*>(g + i) * gs;
            f32x4 M = *reinterpret_cast<f32x4*>(m + i), V = *reinterpret_cast<f32x4*>(v + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                M[k] = b1 * M[k] + (1.f - b1) * G[k];
                V[k] = b2 * V[k] + (1.f - b2) * G[k] * G[k];
                P[k] -= step_size * M[k] / (sqrtf(V[k]) / bc2s + eps);
            }
            *reinterpret_cast<f32x4*>(p + i) = P; *reinterpret_cast<f32x4*>(m + i) = M; *reinterpret_cast<f32x4*>(v + i) = V;
        }
    } else {
        for (int i = threadIdx.x; i < lim; i += NT) {
            float G = g[i] * gs;
            float M = b1 * m[i] + (1.f - b1) * G;
            float V = b2 * v[i] + (1.f - b2) * G * G;
            p[i] -= step_size * M / (sqrtf(V) / bc2s + eps);
            m[i] = M; v[i] = V;
        }
    }
}
__global__ void adam_bump_kernel(const XmcAdamEntry* tab, int n, const int* __restrict__ si) {
    if (si && *si) return;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) *tab[i].step += 1;
}
}  // namespace

extern "C" int xmc_adam_chunk_elems(void) { return CHUNK; }

// ---------------------------------------------------------------------------------------------------------------------------
// Exponential moving average of the weights (the shadow set a GAN is sampled from at evaluation time), once per APPLIED
// optimizer step:  e += (1 - d) * (p - e)  with d = 0 while fewer than `start` updates have been applied (then e = p, a bit-exact
// copy) and d = decay afterwards.  The number of applied updates is ONE device counter for the whole shadow set and the choice
// is made here from it, so a captured graph crosses `start` without re-capture.  The (p - e) form makes e == p a fixed point.
// Unlike adam_kernel above these kernels take 16-byte accesses only where every pointer they dereference is 16-byte aligned
// (chunks start at multiples of CHUNK elements, so a chunk is aligned exactly when its tensors' bases are) and finish a
// vectorised body with a scalar tail, so tensors carved from a flat buffer at any element offset are handled.
namespace {
__device__ __forceinline__ bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }
__device__ __forceinline__ float ema_elem(float e, float p, float w, bool copy) { return copy ? p : __builtin_fmaf(w, p - e, e); }

__global__ void ema_kernel(const XmcEmaEntry* __restrict__ tab, const int2* __restrict__ chunks, float decay, int start,
                           const int* __restrict__ nupd, const int* __restrict__ si) {
    if (si && *si) return;                      // the optimizer step this update belongs to is skipped: the shadow stays
    const int2 c = chunks[blockIdx.x];
    const XmcEmaEntry t = tab[c.x];
    const bool copy = *nupd < start;
    const float w = 1.f - decay;
    const int64_t base = (int64_t)c.y * CHUNK;
    const int lim = (int)(t.n - base < CHUNK ? t.n - base : CHUNK);
    float* e = t.shadow + base; const float* p = t.param + base;
    int body = 0;
    if (aligned16(e) && aligned16(p)) {
        body = lim & ~3;
        for (int i = threadIdx.x * 4; i < body; i += NT * 4) {
            f32x4 E = *reinterpret_cast<f32x4*>(e + i);
            const f32x4 P = *reinterpret_cast<const f32x4*>(p + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) E[k] = ema_elem(E[k], P[k], w, copy);
            *reinterpret_cast<f32x4*>(e + i) = E;
        }
    }
    for (int i = body + threadIdx.x; i < lim; i += NT) e[i] = ema_elem(e[i], p[i], w, copy);
}

// adam_kernel's update with the shadow update applied to the new weight while it is in registers: 8 bytes of extra traffic per
// element instead of the 12 of a pass of its own.  The weights, moments and counters it leaves are bit-identical to
// adam_kernel's.  That takes care: as compiled, adam_kernel's two paths round the moment updates differently -- its 16-byte path
// (tensors with n % 4 == 0) contracts `b * m + t` into one FMA, its scalar path (all other tensors) rounds product and sum
// separately -- so the arithmetic is written out here, contraction off, in both forms, and a tensor gets the form adam_kernel
// gives it (by n % 4), whichever way this kernel accesses its memory.  ema[c.x].shadow == NULL: that tensor has no shadow.
template <bool FMA>
__device__ __forceinline__ float adam_elem(float P, float G, float& M, float& V, float b1, float b2, float step_size, float bc2s,
                                           float eps) {
#pragma clang fp contract(off)
    const float t = (1.f - b1) * G, u = ((1.f - b2) * G) * G;
    M = FMA ? __builtin_fmaf(b1, M, t) : b1 * M + t;
    V = FMA ? __builtin_fmaf(b2, V, u) : b2 * V + u;
    return P - (step_size * M) / (sqrtf(V) / bc2s + eps);
}

template <bool FMA>
__device__ __forceinline__ void adam_ema_chunk(float* p, const float* g, float* m, float* v, float* sh, int lim, float gs, float b1,
                                               float b2, float step_size, float bc2s, float eps, float w, bool copy) {
    int body = 0;
    if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(sh)) {
        body = lim & ~3;
        for (int i = threadIdx.x * 4; i < body; i += NT * 4) {
            f32x4 P = *reinterpret_cast<f32x4*>(p + i), G = *reinterpret_cast<const f32x4*>(g + i);
            f32x4 M = *reinterpret_cast<f32x4*>(m + i), V = *reinterpret_cast<f32x4*>(v + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float Mk = M[k], Vk = V[k];
                P[k] = adam_elem<FMA>(P[k], G[k] * gs, Mk, Vk, b1, b2, step_size, bc2s, eps);
                M[k] = Mk; V[k] = Vk;
            }
            *reinterpret_cast<f32x4*>(p + i) = P; *reinterpret_cast<f32x4*>(m + i) = M; *reinterpret_cast<f32x4*>(v + i) = V;
            if (sh) {
                f32x4 E = *reinterpret_cast<f32x4*>(sh + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) E[k] = ema_elem(E[k], P[k], w, copy);
                *reinterpret_cast<f32x4*>(sh + i) = E;
            }
        }
    }
    for (int i = body + threadIdx.x; i < lim; i += NT) {
        float M = m[i], V = v[i];
        const float P = adam_elem<FMA>(p[i], g[i] * gs, M, V, b1, b2, step_size, bc2s, eps);
        p[i] = P; m[i] = M; v[i] = V;
        if (sh) sh[i] = ema_elem(sh[i], P, w, copy);
    }
}

__global__ void adam_ema_kernel(const XmcAdamEntry* __restrict__ tab, const XmcEmaEntry* __restrict__ ema,
                                const int2* __restrict__ chunks, float lr, float b1, float b2, float eps, float gs,
                                const float* __restrict__ sf, const int* __restrict__ si, float decay, int start,
                                const int* __restrict__ nupd) {
    if (si && *si) return;                      // a non-finite gradient: the whole step is skipped, shadow included
    if (sf) gs *= sf[1];
    const int2 c = chunks[blockIdx.x];
    const XmcAdamEntry t = tab[c.x];
    const int step = *t.step + 1;
    const float bc1 = 1.f - powf(b1, (float)step), bc2s = sqrtf(1.f - powf(b2, (float)step));
    const float step_size = lr / bc1;
    const bool copy = *nupd < start;
    const float w = 1.f - decay;
    const int64_t base = (int64_t)c.y * CHUNK;
    const int lim = (int)(t.n - base < CHUNK ? t.n - base : CHUNK);
    float* sh = ema[c.x].shadow;
    if (sh) sh += base;
    if ((t.n & 3) == 0) adam_ema_chunk<true>(t.param + base, t.grad + base, t.m + base, t.v + base, sh, lim, gs, b1, b2, step_size, bc2s, eps, w, copy);
    else adam_ema_chunk<false>(t.param + base, t.grad + base, t.m + base, t.v + base, sh, lim, gs, b1, b2, step_size, bc2s, eps, w, copy);
}

// after all tensors: the per-tensor Adam counters (tab == NULL: none) and, with `bump`, the shadow set's one counter
__global__ void ema_bump_kernel(const XmcAdamEntry* tab, int n, const int* __restrict__ si, int* nupd, int bump) {
    if (si && *si) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (tab && i < n) *tab[i].step += 1;
    if (bump && i == 0) *nupd += 1;
}

bool ema_args_ok(float decay, int start, const int32_t* nupd) { return nupd && decay >= 0.f && decay < 1.f && start >= 0; }
}  // namespace

extern "C" int xmc_ema_step(const XmcEmaEntry* table_dev, int ntensors, const int32_t* chunks_dev, int nchunks, float decay,
                            int start, int32_t* num_updates_dev, const int32_t* skip_flag_dev, int bump, void* stream) {
    if (!table_dev || !chunks_dev || ntensors < 1 || nchunks < 1 || !ema_args_ok(decay, start, num_updates_dev)) return XMC_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ema_kernel, dim3(nchunks), dim3(NT), 0, st, table_dev, reinterpret_cast<const int2*>(chunks_dev), decay, start,
                       (const int*)num_updates_dev, (const int*)skip_flag_dev);
    if (bump)
        hipLaunchKernelGGL(ema_bump_kernel, dim3(1), dim3(64), 0, st, (const XmcAdamEntry*)nullptr, 0, (const int*)skip_flag_dev,
                           (int*)num_updates_dev, 1);
    XMC_LAUNCH_CHECK();
    return 0;
}


// One optimizer launch group.  The two optional parts are keyed on their pointers: a loss scale on scale_dev / flags_dev, a
// shadow set on ema_table / num_updates_dev.  adam_kernel + adam_bump_kernel without a shadow, adam_ema_kernel + ema_bump_kernel
// with one; the check in front and the rescale behind exist only under a loss scale.
extern "C" int xmc_optim_step(const XmcOptimStep* s, void* stream) {
    if (!s || !s->table || !s->chunks || s->ntensors < 1 || s->nchunks < 1) return XMC_EINVAL;
    const bool scaled = s->scale_dev || s->flags_dev, shadow = s->ema_table || s->num_updates_dev;
    if (scaled ? (!s->scale_dev || !s->flags_dev || s->interval < 1 || (s->mode & 7) == 0 || s->grad_scale != 1.f) : s->mode != XMC_ADAM_UPDATE)
        return XMC_EINVAL;
    if (shadow && (!s->ema_table || !ema_args_ok(s->decay, s->start, s->num_updates_dev))) return XMC_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int2* ch = reinterpret_cast<const int2*>(s->chunks);
    const float* sf = s->scale_dev;
    const int* si = s->flags_dev;
    const dim3 bump_grid((s->ntensors + NT - 1) / NT);
    if (s->mode & XMC_ADAM_CHECK) hipLaunchKernelGGL(adam_check_kernel, dim3(s->nchunks), dim3(NT), 0, st, s->table, ch, s->flags_dev);
    if ((s->mode & XMC_ADAM_UPDATE) && shadow) {
        hipLaunchKernelGGL(adam_ema_kernel, dim3(s->nchunks), dim3(NT), 0, st, s->table, s->ema_table, ch, s->lr, s->beta1, s->beta2, s->eps,
                           s->grad_scale, sf, si, s->decay, s->start, (const int*)s->num_updates_dev);
        hipLaunchKernelGGL(ema_bump_kernel, bump_grid, dim3(NT), 0, st, s->table, s->ntensors, si, (int*)s->num_updates_dev, s->bump);
    } else if (s->mode & XMC_ADAM_UPDATE) {
        hipLaunchKernelGGL(adam_kernel, dim3(s->nchunks), dim3(NT), 0, st, s->table, ch, s->lr, s->beta1, s->beta2, s->eps, s->grad_scale, sf, si);
        hipLaunchKernelGGL(adam_bump_kernel, bump_grid, dim3(NT), 0, st, s->table, s->ntensors, si);
    }
    if (s->mode & XMC_ADAM_RESCALE)
        hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, st, s->scale_dev, s->flags_dev, s->growth, s->backoff, s->interval);
    XMC_LAUNCH_CHECK();
    return 0;
}
