// The rest of the optimizer family over the flat parameter / gradient buffers (include/nmhip_optim.h): pass 3 of
// nm_optim.hip -- per-tensor clip + update -- for TF 1.12's ApplyGradientDescent, ApplyMomentum, ApplyAdagrad and
// ApplyRMSProp.  Passes 1 and 2 (regulariser terms, per-variable norms) are nm_optim.hip's and leave the squared norms
// in the workspace this pass reads its clip scale from.  A kind touches only the streams it has:
//   2 GradientDescent  theta, g              -> theta                 var -= lr*g
//   3 Momentum         theta, g, accum       -> theta, accum          accum = accum*mu + g; var -= lr*accum
//                                                                     (Nesterov: var -= g*lr + accum*mu*lr)
//   4 Adagrad          theta, g, accum       -> theta, accum          accum += g*g; var -= g*lr*rsqrt(accum)
//   5 RMSProp          theta, g, ms, mom     -> theta, ms, mom        ms += (g*g - ms)*(1-decay);
//                                                                     mom = mom*mu + (g*lr)/sqrt(ms + eps); var -= mom
#include "nm_common.h"
#include "../../include/nmhip_optim.h"

extern "C" int64_t nm_optim_workspace_bytes(int64_t nchunk, int64_t nseg);      // nm_optim.hip

namespace {

struct FamilyChunks {
    const long* chunk_start;   // [nchunk] flat offset
    const int* chunk_len;      // [nchunk]
    const int* chunk_seg;      // [nchunk]
    const int* seg_flags;      // [nseg] bit0 regularizable, bit1 trainable
};

// one element of kind KIND: th, a, b are updated in place (a, b: the slots the kind has)
template <int KIND>
__device__ __forceinline__ void family_one(float& th, float g, float& a, float& b, float p0, float p1, float p2,
                                           float p3) {
    if (KIND == NM_OPTIM_SGD) {
        th -= p0 * g;
    } else if (KIND == NM_OPTIM_MOMENTUM) {                 // p0 lr, p1 momentum, p2 != 0: Nesterov
        a = a * p1 + g;
        if (p2 != 0.0f) th -= g * p0 + a * p1 * p0;
        else th -= p0 * a;
    } else if (KIND == NM_OPTIM_ADAGRAD) {                  // p0 lr
        a += g * g;
        th -= g * p0 * (1.0f / sqrtf(a));
    } else {                                                // RMSProp: p0 lr, p1 decay, p2 momentum, p3 epsilon
        a += (g * g - a) * (1.0f - p1);
        b = b * p2 + (g * p0) / sqrtf(a + p3);
        th -= b;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void opt_family_kernel(FamilyChunks t, float* __restrict__ theta,
                                                         const float* __restrict__ grad, float* __restrict__ s0,
                                                         float* __restrict__ s1, const float* __restrict__ seg_norm2,
                                                         float clip, float p0, float p1, float p2, float p3, int c0,
                                                         const int* __restrict__ skip, const int* __restrict__ list) {
    constexpr bool HAS0 = KIND != NM_OPTIM_SGD, HAS1 = KIND == NM_OPTIM_RMSPROP;
    if (skip && *skip != 0) return;          // the step's gradient is garbage (a time loop gave up): nothing is applied
    const int c = list ? list[blockIdx.x] : c0 + (int)blockIdx.x;
    const int seg = t.chunk_seg[c];
    if (!(t.seg_flags[seg] & 2)) return;
    const long base = t.chunk_start[c];
    const int len = t.chunk_len[c];
    float scale = 1.0f;
    if (clip > 0.0f) scale = clip / fmaxf(sqrtf(seg_norm2[seg]), clip);
    int done = 0;
    if ((base & 3) == 0) {                   // 16-byte rows (every variable starts on one; a shard's cut may not)
        const int len4 = len >> 2;
        float4* th4 = reinterpret_cast<float4*>(theta + base);
        const float4* g4 = reinterpret_cast<const float4*>(grad + base);
        float4* a4 = HAS0 ? reinterpret_cast<float4*>(s0 + base) : nullptr;
        float4* b4 = HAS1 ? reinterpret_cast<float4*>(s1 + base) : nullptr;
        for (int i = threadIdx.x; i < len4; i += 256) {
            float4 th = th4[i];
            const float4 g = g4[i];
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
            if (HAS0) a = a4[i];
            if (HAS1) b = b4[i];
            family_one<KIND>(th.x, g.x * scale, a.x, b.x, p0, p1, p2, p3);
            family_one<KIND>(th.y, g.y * scale, a.y, b.y, p0, p1, p2, p3);
            family_one<KIND>(th.z, g.z * scale, a.z, b.z, p0, p1, p2, p3);
            family_one<KIND>(th.w, g.w * scale, a.w, b.w, p0, p1, p2, p3);
            if (HAS0) a4[i] = a;
            if (HAS1) b4[i] = b;
            th4[i] = th;
        }
        done = len4 << 2;
    }
    for (int i = done + threadIdx.x; i < len; i += 256) {
        float th = theta[base + i], a = 0.0f, b = 0.0f;
        if (HAS0) a = s0[base + i];
        if (HAS1) b = s1[base + i];
        family_one<KIND>(th, grad[base + i] * scale, a, b, p0, p1, p2, p3);
        if (HAS0) s0[base + i] = a;
        if (HAS1) s1[base + i] = b;
        theta[base + i] = th;
    }
}

// everything both entry points refuse; ``who`` names the function in the text
int family_check(const char* who, int32_t kind, const float* theta, const float* grad, const float* slot0,
                 const float* slot1, const void* chunk_start, const void* chunk_len, const void* chunk_seg,
                 const void* seg_first, const void* seg_count, const void* seg_flags, int64_t nchunk, int64_t nseg,
                 const void* workspace, int64_t workspace_bytes) {
    NM_REQUIRE(kind >= NM_OPTIM_SGD && kind <= NM_OPTIM_RMSPROP,
               "%s: kind %d (2 GradientDescent, 3 Momentum, 4 Adagrad, 5 RMSProp)", who, (int)kind);
    NM_REQUIRE(theta && grad && workspace, "%s: null theta, grad or workspace", who);
    NM_REQUIRE(chunk_start && chunk_len && chunk_seg && seg_first && seg_count && seg_flags, "%s: null table", who);
    NM_REQUIRE(kind == NM_OPTIM_SGD || slot0, "%s: kind %d needs slot0", who, (int)kind);
    NM_REQUIRE(kind != NM_OPTIM_RMSPROP || slot1, "%s: kind %d needs slot1", who, (int)kind);
    NM_REQUIRE(nchunk > 0 && nseg > 0 && nchunk <= 0x7fffffff, "%s: bad sizes nchunk %ld, nseg %ld", who, (long)nchunk,
               (long)nseg);
    if (workspace_bytes < nm_optim_workspace_bytes(nchunk, nseg))
        NM_FAIL(NM_ERR_WORKSPACE, "%s: workspace of %ld bytes, %ld needed", who, (long)workspace_bytes,
                (long)nm_optim_workspace_bytes(nchunk, nseg));
    return NM_OK;
}

void family_launch(void* stream, int32_t kind, unsigned grid, FamilyChunks t, float* theta, const float* grad,
                   float* slot0, float* slot1, const float* seg_norm2, float clip, float p0, float p1, float p2, float p3,
                   int c0, const int* skip, const int* list) {
    hipStream_t s = nm_stream(stream);
    // a slot the kind does not have never reaches its kernel
    switch (kind) {
    case NM_OPTIM_SGD:
        hipLaunchKernelGGL(opt_family_kernel<NM_OPTIM_SGD>, dim3(grid), dim3(256), 0, s, t, theta, grad,
                           (float*)nullptr, (float*)nullptr, seg_norm2, clip, p0, p1, p2, p3, c0, skip, list);
        break;
    case NM_OPTIM_MOMENTUM:
        hipLaunchKernelGGL(opt_family_kernel<NM_OPTIM_MOMENTUM>, dim3(grid), dim3(256), 0, s, t, theta, grad, slot0,
                           (float*)nullptr, seg_norm2, clip, p0, p1, p2, p3, c0, skip, list);
        break;
    case NM_OPTIM_ADAGRAD:
        hipLaunchKernelGGL(opt_family_kernel<NM_OPTIM_ADAGRAD>, dim3(grid), dim3(256), 0, s, t, theta, grad, slot0,
                           (float*)nullptr, seg_norm2, clip, p0, p1, p2, p3, c0, skip, list);
        break;
    default:
        hipLaunchKernelGGL(opt_family_kernel<NM_OPTIM_RMSPROP>, dim3(grid), dim3(256), 0, s, t, theta, grad, slot0,
                           slot1, seg_norm2, clip, p0, p1, p2, p3, c0, skip, list);
    }
}

FamilyChunks family_chunks(const int64_t* chunk_start, const int32_t* chunk_len, const int32_t* chunk_seg,
                           const int32_t* seg_flags) {
    FamilyChunks t;
    t.chunk_start = reinterpret_cast<const long*>(chunk_start);
    t.chunk_len = chunk_len; t.chunk_seg = chunk_seg; t.seg_flags = seg_flags;
    return t;
}

}  // namespace

extern "C" int nm_optim_update(void* stream, int32_t kind, float* theta, const float* grad, float* slot0, float* slot1,
                               const int64_t* chunk_start, const int32_t* chunk_len, const int32_t* chunk_seg,
                               const int32_t* seg_first, const int32_t* seg_count, const int32_t* seg_flags,
                               int64_t nchunk, int64_t nseg, float clip_norm, float p0, float p1, float p2, float p3,
                               int64_t chunk_begin, int64_t chunk_end, const int32_t* skip_word, void* workspace,
                               int64_t workspace_bytes) {
    const int rc = family_check("nm_optim_update", kind, theta, grad, slot0, slot1, chunk_start, chunk_len, chunk_seg,
                                seg_first, seg_count, seg_flags, nchunk, nseg, workspace, workspace_bytes);
    if (rc != NM_OK) return rc;
    NM_REQUIRE(chunk_begin >= 0 && chunk_begin <= chunk_end && chunk_end <= nchunk,
               "nm_optim_update: bad chunk range [%ld, %ld) of %ld", (long)chunk_begin, (long)chunk_end, (long)nchunk);
    if (chunk_begin == chunk_end) return NM_OK;
    const float* seg_norm2 = reinterpret_cast<const float*>(workspace) + nchunk * 3;
    family_launch(stream, kind, (unsigned)(chunk_end - chunk_begin),
                  family_chunks(chunk_start, chunk_len, chunk_seg, seg_flags), theta, grad, slot0, slot1, seg_norm2,
                  clip_norm, p0, p1, p2, p3, (int)chunk_begin, skip_word, nullptr);
    NM_LAUNCH_CHECK("nm_optim_update");
}

extern "C" int nm_optim_update_list(void* stream, int32_t kind, float* theta, const float* grad, float* slot0,
                                    float* slot1, const int64_t* chunk_start, const int32_t* chunk_len,
                                    const int32_t* chunk_seg, const int32_t* seg_first, const int32_t* seg_count,
                                    const int32_t* seg_flags, int64_t nchunk, int64_t nseg, float clip_norm, float p0,
                                    float p1, float p2, float p3, const int32_t* chunk_list, int64_t count,
                                    const int32_t* skip_word, void* workspace, int64_t workspace_bytes) {
    const int rc = family_check("nm_optim_update_list", kind, theta, grad, slot0, slot1, chunk_start, chunk_len,
                                chunk_seg, seg_first, seg_count, seg_flags, nchunk, nseg, workspace, workspace_bytes);
    if (rc != NM_OK) return rc;
    NM_REQUIRE(count >= 0 && count <= nchunk && (count == 0 || chunk_list),
               "nm_optim_update_list: bad chunk list (%ld of %ld)", (long)count, (long)nchunk);
    if (count == 0) return NM_OK;
    const float* seg_norm2 = reinterpret_cast<const float*>(workspace) + nchunk * 3;
    family_launch(stream, kind, (unsigned)count, family_chunks(chunk_start, chunk_len, chunk_seg, seg_flags), theta,
                  grad, slot0, slot1, seg_norm2, clip_norm, p0, p1, p2, p3, 0, skip_word, chunk_list);
    NM_LAUNCH_CHECK("nm_optim_update_list");
}
