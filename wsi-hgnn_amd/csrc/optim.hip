// The optimizer steps for gfx950: ONE launch over all parameters of the model (the step the reference's trainer takes after loss.backward():
// torch.optim.Adam(lr, weight_decay) of parser.py:33-38, trainer/train_gnn.py:72; Adagrad, Adadelta and SGD are parser.py:15-46's other branches).
// Contract: include/wsi_hgnn.h.
//
// One kernel template over the rule.  HBM-bound streaming, 16-byte lane accesses where every pointer of the tensor allows it; the tensor table
// travels in the kernel arguments (no upload); a workgroup of 256 threads takes 4096 elements and finds its tensor by a scan of the block prefix.
// HBM bytes per element (read + written): SGD 8 + 4, SGD with momentum 12 + 8 (8 + 8 on a tensor's first step), Adagrad 12 + 8,
// Adadelta 16 + 12, Adam 16 + 12.
//
// The device step count.  A tensor with a `step` word: lane 0 of each workgroup loads the old count, the factors that depend on t = old + 1
// (Adam's two bias corrections, Adagrad's clr) are computed from it in double by that one lane and handed to the workgroup through LDS.  When
// the workgroup has issued its elements, lane 0 draws a ticket (one returning relaxed agent-scope add on the tensor's ticket word); whoever
// draws the last one stores old + 1 and swaps the ticket back to 0.  Nobody waits for anybody: a workgroup has CONSUMED its load of the count
// (it went through LDS and a barrier) before its add issues, so the one store of the new count comes after every load of the old one, and
// what this launch writes (elements, count, ticket) is read by the next kernel only - no fence.
//
// The learning rate as a device word (wsi_optim_step_lr).  The kernel template has a second parameter, WORD: the five WORD = false instances
// are the kernels of wsi_optim_step / wsi_optim_step_gated, instruction for instruction what they were before the word existed (T.lr stays a
// scalar load of the kernel arguments, SGD without a step word stays without a barrier); the five WORD = true instances let the lane that
// loads the count load the 8-byte word too and form from it, in double and in optim_factors' order, what is made of lr - the (float)lr of
// SGD and Adadelta, Adam's step_size, Adagrad's clr - and hand it over in the LDS word that carries f0.  The word is written by the host's
// fill_ on the same stream between launches and only read here: a plain load.
#include "common.h"
#include <math.h>
#include <cmath>

namespace wsi {

constexpr int OPTIM_MAX = 88;             // tensors per launch (HEATNet4 with 3 node types has 75); see the static_assert below
constexpr int OPTIM_BLOCK_ELEMS = 4096;   // elements per workgroup (256 threads x 4 vectors of 4)
enum { R_SGD = 0, R_SGD_MOMENTUM, R_ADAGRAD, R_ADADELTA, R_ADAM };      // (kernel instances: SGD without a buffer is one of its own)

struct OptimTable {
    float* p[OPTIM_MAX];
    const float* g[OPTIM_MAX];
    float* s0[OPTIM_MAX];
    float* s1[OPTIM_MAX];
    float* step[OPTIM_MAX];
    int32_t* ticket[OPTIM_MAX];
    int64_t n[OPTIM_MAX];
    int32_t block_start[OPTIM_MAX + 1];
    uint8_t flags[OPTIM_MAX];
    uint8_t gate[OPTIM_MAX];                              // 0: no gate; k: the tensor is stepped only when gate_table[k - 1] != 0 (wsi_optim_step_gated)
    int32_t count;
    double lr_d, lr_decay_d, beta1_d, beta2_d;            // what the t-dependent factors are made of, in double
    float lr, weight_decay, momentum, omd, eps, rho, omr, beta2, omb1, omb2;     // omd = 1 - dampening, omr = 1 - rho, omb = 1 - beta
    float f0, f1;                                         // the factors for t = host_step: Adam step_size, bc2_sqrt; Adagrad clr
    int32_t nesterov;
    const float* gate_table;                              // device words, read by every workgroup of a gated tensor
    const double* lr_word;                                // wsi_optim_step_lr: one device double read by lane 0 of every workgroup in place of lr_d / lr (else null)
};
static_assert(sizeof(OptimTable) <= 5680, "the table travels in the kernel arguments: no larger than the largest argument block this library has "
                                          "launched with (5680 bytes: the 128-tensor table of the Adam kernel this template replaced)");

// the factors of the 1-based count t (double in, float out): the host for host_step, lane 0 of a workgroup for a device count
template <int RULE>
__host__ __device__ __forceinline__ void optim_factors(double t, double lr, double lr_decay, double beta1, double beta2, float& f0, float& f1) {
    if (RULE == R_ADAM) {
        f0 = (float)(lr / (1.0 - pow(beta1, t)));
        f1 = (float)sqrt(1.0 - pow(beta2, t));
    } else if (RULE == R_ADAGRAD) {
        f0 = (float)(lr / (1.0 + (t - 1.0) * lr_decay));
        f1 = 0.f;
    } else {
        f0 = f1 = 0.f;
    }
}

// one element, torch's order of operations (products that torch rounds on their own in a kernel of their own are rounded here too)
template <int RULE>
__device__ __forceinline__ void optim_one(float& p, float g, float& a, float& b, const OptimTable& T, float lr, float f0, float f1, bool first) {
    g = fmaf(T.weight_decay, p, g);                                        // every rule: L2 penalty added to the gradient
    if (RULE == R_SGD) {
        p = fmaf(-lr, g, p);
    } else if (RULE == R_SGD_MOMENTUM) {
        a = first ? g : fmaf(T.omd, g, __fmul_rn(T.momentum, a));          // buf.mul_(momentum).add_(grad, alpha=1 - dampening); first step: buf = grad
        g = T.nesterov ? fmaf(T.momentum, a, g) : a;
        p = fmaf(-lr, g, p);
    } else if (RULE == R_ADAGRAD) {
        a = fmaf(g, g, a);                                                 // state_sum.addcmul_(grad, grad, value=1)
        p = fmaf(-f0, g / (sqrtf(a) + T.eps), p);                          // param.addcdiv_(grad, sqrt(sum) + eps, value=-clr)
    } else if (RULE == R_ADADELTA) {
        a = fmaf(__fmul_rn(T.omr, g), g, __fmul_rn(T.rho, a));             // square_avg.mul_(rho).addcmul_(grad, grad, value=1 - rho)
        const float d = __fmul_rn(sqrtf(b + T.eps) / sqrtf(a + T.eps), g); // delta = sqrt(acc_delta + eps) / sqrt(square_avg + eps) * grad
        b = fmaf(__fmul_rn(T.omr, d), d, __fmul_rn(T.rho, b));             // acc_delta.mul_(rho).addcmul_(delta, delta, value=1 - rho)
        p = fmaf(-lr, d, p);
    } else {                                                               // Adam: step_size = f0, bc2_sqrt = f1
        a = fmaf(T.omb1, g - a, a);
        b = fmaf(T.beta2, b, T.omb2 * g * g);
        const float denom = sqrtf(b) / f1 + T.eps;
        p -= f0 * (a / denom);
    }
}

template <int RULE, bool WORD>
__global__ __launch_bounds__(256) void optim_step_kernel(const OptimTable T) {
    constexpr int NS = RULE == R_SGD ? 0 : (RULE == R_SGD_MOMENTUM || RULE == R_ADAGRAD) ? 1 : 2;        // state tensors of the rule
    __shared__ float s_t[3];                                               // old count, f0, f1 of this workgroup's tensor
    int t = 0;
    const int blk = (int)blockIdx.x;
    while (t + 1 < T.count && T.block_start[t + 1] <= blk) ++t;            // (block-uniform)
    t = __builtin_amdgcn_readfirstlane(t);                                 // (said to the compiler: every table read below stays a scalar load of the kernel arguments)
    // a gated tensor whose gate word is 0.0: the whole workgroup leaves before it loads, stores or takes a ticket (block-uniform, in front of
    // every barrier) - p, the states, the count and the ticket word stay as they were, as torch leaves a parameter without a gradient
    const int gate = T.gate[t];
    if (gate && T.gate_table[gate - 1] == 0.f) return;
    const int64_t base = (int64_t)(blk - T.block_start[t]) * OPTIM_BLOCK_ELEMS;
    const int64_t n = T.n[t];
    float* __restrict__ p = T.p[t];
    const float* __restrict__ g = T.g[t];
    float* __restrict__ s0 = T.s0[t];
    float* __restrict__ s1 = T.s1[t];
    float* const step = T.step[t];
    const bool first = (T.flags[t] & WSI_OPTIM_FIRST) != 0;
    constexpr bool COUNTS = RULE == R_ADAM || RULE == R_ADAGRAD;             // the rules that read t
    float f0 = 0.f, f1 = 0.f, old = 0.f;
    if (WORD || COUNTS || step) {                                          // (block-uniform; the factors reach the lanes through LDS on both paths:
        if (threadIdx.x == 0) {                                            //  a choice between an LDS word and a kernel argument would cost a copy of the table)
            float a0 = T.f0, a1 = T.f1;                                    // t = host_step: taken on the host
            const double lr_d = WORD ? *T.lr_word : T.lr_d;                // (a rule that reads t takes a word with a step word only: the host checked)
            if (step) {
                old = __hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                optim_factors<RULE>((double)old + 1.0, lr_d, T.lr_decay_d, T.beta1_d, T.beta2_d, a0, a1);
            }
            if (WORD && !COUNTS) a0 = (float)lr_d;                         // SGD, Adadelta: what the host puts into T.lr, rounded the same way
            s_t[0] = old; s_t[1] = a0; s_t[2] = a1;
        }
        __syncthreads();
        f0 = s_t[1]; f1 = s_t[2];
    }
    const float lr = WORD ? f0 : T.lr;                                     // (read by SGD and Adadelta only)
    uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g);
    if (NS >= 1) bits |= reinterpret_cast<uintptr_t>(s0);
    if (NS >= 2) bits |= reinterpret_cast<uintptr_t>(s1);
    const bool vec = (bits & 15) == 0;
#pragma unroll
    for (int q = 0; q < OPTIM_BLOCK_ELEMS / 1024; ++q) {
        const int64_t i = base + q * 1024 + (int64_t)threadIdx.x * 4;
        if (i >= n) break;
        if (vec && i + 3 < n) {
            float4 pv = *reinterpret_cast<const float4*>(p + i);
            const float4 gv = *reinterpret_cast<const float4*>(g + i);
            float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
            if (NS >= 1 && !(RULE == R_SGD_MOMENTUM && first)) av = *reinterpret_cast<const float4*>(s0 + i);
            if (NS >= 2) bv = *reinterpret_cast<const float4*>(s1 + i);
            optim_one<RULE>(pv.x, gv.x, av.x, bv.x, T, lr, f0, f1, first); optim_one<RULE>(pv.y, gv.y, av.y, bv.y, T, lr, f0, f1, first);
            optim_one<RULE>(pv.z, gv.z, av.z, bv.z, T, lr, f0, f1, first); optim_one<RULE>(pv.w, gv.w, av.w, bv.w, T, lr, f0, f1, first);
            *reinterpret_cast<float4*>(p + i) = pv;
            if (NS >= 1) *reinterpret_cast<float4*>(s0 + i) = av;
            if (NS >= 2) *reinterpret_cast<float4*>(s1 + i) = bv;
        } else {
            for (int k = 0; k < 4 && i + k < n; ++k) {
                float pk = p[i + k], ak = 0.f, bk = 0.f;
                if (NS >= 1 && !(RULE == R_SGD_MOMENTUM && first)) ak = s0[i + k];
                if (NS >= 2) bk = s1[i + k];
                optim_one<RULE>(pk, g[i + k], ak, bk, T, lr, f0, f1, first);
                p[i + k] = pk;
                if (NS >= 1) s0[i + k] = ak;
                if (NS >= 2) s1[i + k] = bk;
            }
        }
    }
    if (step && threadIdx.x == 0) {                                        // (`old` is lane 0's own register: loaded above, before the barrier)
        int32_t* const ticket = T.ticket[t];
        const int32_t blocks = T.block_start[t + 1] - T.block_start[t];
        if (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == blocks - 1) {
            __hip_atomic_store(step, old + 1.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_exchange(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int RULE>
static void optim_launch(const OptimTable& T, unsigned blocks, hipStream_t st) {
    if (T.lr_word) hipLaunchKernelGGL((optim_step_kernel<RULE, true>), dim3(blocks), dim3(256), 0, st, T);
    else hipLaunchKernelGGL((optim_step_kernel<RULE, false>), dim3(blocks), dim3(256), 0, st, T);
}

}  // namespace wsi

using namespace wsi;

// the kernel instance of a rule, and the state tensors it reads (s0, s1)
static int optim_instance(int32_t rule, const wsi_optim_hyper_t& H) {
    return rule == WSI_OPTIM_SGD ? (H.momentum != 0.0 ? R_SGD_MOMENTUM : R_SGD) : rule == WSI_OPTIM_ADAGRAD ? R_ADAGRAD : rule == WSI_OPTIM_ADADELTA ? R_ADADELTA : R_ADAM;
}
static int optim_states(int inst) { return inst == R_SGD ? 0 : (inst == R_SGD_MOMENTUM || inst == R_ADAGRAD) ? 1 : 2; }

// What the entry points do once every argument is checked: the hyper-parameters into the table, then one launch per OPTIM_MAX non-empty tensors.
// gate_index: per tensor 0 (no gate) or the 1-based word of gate_table; null: no tensor is gated.
static void optim_launches(int32_t rule, const wsi_optim_tensor_t* tensors, int32_t count, const wsi_optim_hyper_t& H, hipStream_t st,
                           const int32_t* gate_index = nullptr, const float* gate_table = nullptr, const double* lr_word = nullptr) {
    const int inst = optim_instance(rule, H), ns = optim_states(inst);
    OptimTable T;
    T.lr_d = H.lr; T.lr_decay_d = H.lr_decay; T.beta1_d = H.beta1; T.beta2_d = H.beta2;
    // the scalar factors in double, as torch's host code takes them (1 - 0.999f in float is off by 1.3e-5 relative)
    T.lr = (float)H.lr; T.weight_decay = (float)H.weight_decay; T.momentum = (float)H.momentum; T.omd = (float)(1.0 - H.dampening);
    T.eps = (float)H.eps; T.rho = (float)H.rho; T.omr = (float)(1.0 - H.rho);
    T.beta2 = (float)H.beta2; T.omb1 = (float)(1.0 - H.beta1); T.omb2 = (float)(1.0 - H.beta2);
    T.nesterov = H.nesterov != 0.0;
    T.f0 = T.f1 = 0.f;
    T.gate_table = gate_table;
    T.lr_word = lr_word;
    if (H.host_step >= 1.0) {
        if (inst == R_ADAM) optim_factors<R_ADAM>(H.host_step, H.lr, H.lr_decay, H.beta1, H.beta2, T.f0, T.f1);
        if (inst == R_ADAGRAD) optim_factors<R_ADAGRAD>(H.host_step, H.lr, H.lr_decay, H.beta1, H.beta2, T.f0, T.f1);
    }
    for (int32_t first = 0; first < count;) {          // (`first` advances by what the table CONSUMED: empty tensors are skipped without taking a slot)
        T.count = 0;
        int64_t blocks = 0;
        int32_t i = first;
        for (; i < count && T.count < OPTIM_MAX; ++i) {
            const wsi_optim_tensor_t& a = tensors[i];
            if (a.n == 0) continue;
            const int k = T.count++;
            T.p[k] = a.p; T.g[k] = a.g; T.s0[k] = ns >= 1 ? a.s0 : nullptr; T.s1[k] = ns >= 2 ? a.s1 : nullptr;
            T.step[k] = a.step; T.ticket[k] = a.ticket; T.n[k] = a.n; T.flags[k] = (uint8_t)(a.flags & WSI_OPTIM_FIRST);
            T.gate[k] = gate_index ? (uint8_t)gate_index[i] : 0;
            T.block_start[k] = (int32_t)blocks;
            blocks += (a.n + OPTIM_BLOCK_ELEMS - 1) / OPTIM_BLOCK_ELEMS;
        }
        T.block_start[T.count] = (int32_t)blocks;
        if (T.count) {
            switch (inst) {
                case R_SGD: optim_launch<R_SGD>(T, (unsigned)blocks, st); break;
                case R_SGD_MOMENTUM: optim_launch<R_SGD_MOMENTUM>(T, (unsigned)blocks, st); break;
                case R_ADAGRAD: optim_launch<R_ADAGRAD>(T, (unsigned)blocks, st); break;
                case R_ADADELTA: optim_launch<R_ADADELTA>(T, (unsigned)blocks, st); break;
                default: optim_launch<R_ADAM>(T, (unsigned)blocks, st); break;
            }
        }
        first = i;
    }
}

extern "C" int wsi_adam_step(const wsi_adam_tensor_t* tensors, int32_t count, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int64_t step, void* stream) {
    // wsi_optim_step(WSI_OPTIM_ADAM) with a host count; like it, every tensor is checked before the first launch
    if (count < 0 || step <= 0 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) { set_error("adam_step: bad argument"); return WSI_EINVAL; }
    if (count == 0) return WSI_OK;
    if (!tensors) { set_error("adam_step: null tensor table"); return WSI_EINVAL; }
    int64_t all_blocks = 0;
    for (int32_t i = 0; i < count; ++i) {
        const wsi_adam_tensor_t& a = tensors[i];
        if (a.n < 0 || (a.n > 0 && (!a.p || !a.g || !a.m || !a.v))) { set_error("adam_step: tensor %d: null pointer or negative size", i); return WSI_EINVAL; }
        all_blocks += a.n / OPTIM_BLOCK_ELEMS + 1;
        if (all_blocks > INT32_MAX) { set_error("adam_step: too many elements in one call"); return WSI_EINVAL; }
    }
    wsi_optim_hyper_t H = {};
    H.lr = lr; H.weight_decay = weight_decay; H.eps = eps; H.beta1 = beta1; H.beta2 = beta2; H.host_step = (double)step;
    wsi_optim_tensor_t chunk[OPTIM_MAX];               // the descriptors of one launch, translated (s0 = m, s1 = v, no step word)
    for (int32_t i = 0; i < count;) {
        int32_t k = 0;
        for (; i < count && k < OPTIM_MAX; ++i) {
            const wsi_adam_tensor_t& a = tensors[i];
            if (a.n) chunk[k++] = wsi_optim_tensor_t{a.p, a.g, a.m, a.v, nullptr, nullptr, a.n, 0};
        }
        if (k) optim_launches(WSI_OPTIM_ADAM, chunk, k, H, (hipStream_t)stream);
    }
    return check_launch("adam_step");
}

static int optim_step_checked(int32_t rule, const wsi_optim_tensor_t* tensors, int32_t count, const wsi_optim_hyper_t* hyper,
                              const int32_t* gate_index, const float* gate_table, const double* lr_word, void* stream) {
    // every argument is checked before the first launch: a bad tensor 200 must not leave tensors 0..87 stepped
    if (rule != WSI_OPTIM_SGD && rule != WSI_OPTIM_ADAGRAD && rule != WSI_OPTIM_ADADELTA && rule != WSI_OPTIM_ADAM) { set_error("optim_step: unknown rule %d", rule); return WSI_EINVAL; }
    if (count < 0) { set_error("optim_step: negative tensor count"); return WSI_EINVAL; }
    if (!hyper) { set_error("optim_step: null hyper-parameters"); return WSI_EINVAL; }
    const wsi_optim_hyper_t& H = *hyper;
    // with a word, hyper->lr is ignored: the rate is on the device, where the host cannot look (and the kernel does not, as torch checks no tensor lr)
    bool ok = (lr_word || (std::isfinite(H.lr) && H.lr >= 0.0)) && std::isfinite(H.weight_decay) && H.weight_decay >= 0.0;
    if (rule == WSI_OPTIM_SGD)
        ok = ok && std::isfinite(H.momentum) && H.momentum >= 0.0 && std::isfinite(H.dampening) && (H.nesterov == 0.0 || H.nesterov == 1.0) &&
             (H.nesterov == 0.0 || (H.momentum > 0.0 && H.dampening == 0.0));
    if (rule == WSI_OPTIM_ADAGRAD) ok = ok && std::isfinite(H.lr_decay) && H.lr_decay >= 0.0 && std::isfinite(H.eps) && H.eps >= 0.0;
    if (rule == WSI_OPTIM_ADADELTA) ok = ok && H.rho >= 0.0 && H.rho <= 1.0 && std::isfinite(H.eps) && H.eps >= 0.0;
    if (rule == WSI_OPTIM_ADAM) ok = ok && H.beta1 >= 0.0 && H.beta1 < 1.0 && H.beta2 >= 0.0 && H.beta2 < 1.0 && std::isfinite(H.eps) && H.eps >= 0.0;
    if (!ok) { set_error("optim_step: hyper-parameter out of range"); return WSI_EINVAL; }
    if (count == 0) return WSI_OK;
    if (!tensors) { set_error("optim_step: null tensor table"); return WSI_EINVAL; }
    const bool counts = rule == WSI_OPTIM_ADAGRAD || rule == WSI_OPTIM_ADAM;           // the rules that read t
    const int ns = optim_states(optim_instance(rule, H));
    int64_t all_blocks = 0;
    int32_t nonempty = 0;
    for (int32_t i = 0; i < count; ++i) {
        const wsi_optim_tensor_t& a = tensors[i];
        if (a.n < 0) { set_error("optim_step: tensor %d: negative size", i); return WSI_EINVAL; }
        all_blocks += a.n / OPTIM_BLOCK_ELEMS + 1;
        if (all_blocks > INT32_MAX) { set_error("optim_step: too many elements in one call"); return WSI_EINVAL; }
        if (a.step && !a.ticket) { set_error("optim_step: tensor %d: a step word without a ticket word", i); return WSI_EINVAL; }
        if (a.n == 0) continue;
        ++nonempty;
        if (!a.p || !a.g || (ns >= 1 && !a.s0) || (ns >= 2 && !a.s1)) { set_error("optim_step: tensor %d: null pointer (p, g or a state tensor of the rule)", i); return WSI_EINVAL; }
        if (counts && !a.step && lr_word) { set_error("optim_step_lr: tensor %d has no step word: with a host count the factors are taken on the host, which cannot read the lr word", i); return WSI_EINVAL; }
        if (counts && !a.step && !(H.host_step >= 1.0 && std::isfinite(H.host_step))) { set_error("optim_step: tensor %d has no step word and host_step is not a count >= 1", i); return WSI_EINVAL; }
        if (counts && !a.step && gate_index && gate_index[i]) { set_error("optim_step_gated: tensor %d is gated and has no step word (a host count advances whether it is stepped or not)", i); return WSI_EINVAL; }
    }
    if (nonempty == 0) return WSI_OK;                  // zero-element tensors only: nothing to launch (and no HIP call)
    optim_launches(rule, tensors, count, H, (hipStream_t)stream, gate_index, gate_table, lr_word);
    return check_launch("optim_step");
}

extern "C" int wsi_optim_step(int32_t rule, const wsi_optim_tensor_t* tensors, int32_t count, const wsi_optim_hyper_t* hyper, void* stream) {
    return optim_step_checked(rule, tensors, count, hyper, nullptr, nullptr, nullptr, stream);
}

extern "C" int wsi_optim_step_lr(int32_t rule, const wsi_optim_tensor_t* tensors, int32_t count, const wsi_optim_hyper_t* hyper,
                                 const int32_t* gate_index, const float* gate_table, int32_t gate_len, const double* lr_word, void* stream) {
    if (gate_len < 0 || gate_len > 255) { set_error("optim_step_gated: gate_len %d outside 0..255", gate_len); return WSI_EINVAL; }
    bool any = false;
    for (int32_t i = 0; gate_index && i < count; ++i) {
        if (gate_index[i] < 0 || gate_index[i] > gate_len) { set_error("optim_step_gated: tensor %d: gate index %d outside 0..%d", i, gate_index[i], gate_len); return WSI_EINVAL; }
        any = any || gate_index[i] != 0;
    }
    if (any && !gate_table) { set_error("optim_step_gated: null gate table"); return WSI_EINVAL; }
    if (reinterpret_cast<uintptr_t>(lr_word) & 7) { set_error("optim_step_lr: the lr word is not 8-byte aligned"); return WSI_EINVAL; }
    return optim_step_checked(rule, tensors, count, hyper, any ? gate_index : nullptr, gate_table, lr_word, stream);
}

extern "C" int wsi_optim_step_gated(int32_t rule, const wsi_optim_tensor_t* tensors, int32_t count, const wsi_optim_hyper_t* hyper,
                                    const int32_t* gate_index, const float* gate_table, int32_t gate_len, void* stream) {
    return wsi_optim_step_lr(rule, tensors, count, hyper, gate_index, gate_table, gate_len, nullptr, stream);
}
