// Host side of llm_qat_amd.rope.rotary as a C++ autograd node (PyTorch extension `_fq_rope_node`, optional accelerator of rope.py).
//
// What it replaces: rope._Rotary (a Python torch.autograd.Function).  Why: the two kernels take a few tens of microseconds on a 7B
// layer's q and k, so the host work in front of each launch is a large share of the fused call's time (DESIGN.md section 28 has the A/B);
// the Python Function runs its backward on the autograd engine's thread under the GIL.  This node's forward is two allocations and one
// call through the C ABI, its backward the same.
//
// What it does not do: check arguments.  rope.rotary has run ops.check_rope (types, dtypes, shapes, devices, the CPU dispatch) and hands
// over the tables as [P, D] rows and the positions contiguous; the layout rule of q, k and the gradients is ops._rope_served restated
// (served below).  The kernels are reached through the function pointers of the C ABI (include/llmqat_fakequant_rope.h) that
// _rope_node.py hands over: this file links against PyTorch, not against the HIP library.  Results are the Python node's bit for bit:
// the same entry points with the same arguments.
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <atomic>

#include "../../include/llmqat_fakequant_rope.h"

namespace {

using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

decltype(&fqr_rope_fwd) g_fwd = nullptr;
decltype(&fqr_rope_bwd) g_bwd = nullptr;
decltype(&fqr_rope_dense_strides) g_dense = nullptr;
decltype(&fq_last_error) g_last_error = nullptr;

// what ops.rope_counts adds to its own counts
std::atomic<int64_t> g_fwd_launch{0}, g_bwd_launch{0}, g_copy_route{0};

inline int dtype_code(c10::ScalarType t) {
    return t == at::kFloat ? FQ_DTYPE_F32 : t == at::kBFloat16 ? FQ_DTYPE_BF16 : t == at::kHalf ? FQ_DTYPE_F16 : -1;
}

// ops._rope_served: a tensor whose last stride is 1 is read where it lies; anything else is copied once and counted
inline at::Tensor served(const at::Tensor& t) {
    if (t.stride(3) == 1 || t.size(3) == 1) return t;
    g_copy_route.fetch_add(1, std::memory_order_relaxed);
    return t.contiguous();
}

// the dense result of an input of the given sizes and strides: ops.rope_dense_like and an empty_strided
inline at::Tensor dense_like(c10::IntArrayRef sizes, c10::IntArrayRef strides, const at::TensorOptions& opt) {
    int64_t s[3];
    const int rc = g_dense(sizes[0], sizes[1], sizes[2], sizes[3], strides[0], strides[1], strides[2], s);
    TORCH_CHECK(rc == FQ_OK, "rope_dense_like failed (code ", rc, "): ", g_last_error ? g_last_error() : "");
    return at::empty_strided(sizes, {s[0], s[1], s[2], 1}, opt);
}

struct RotaryNode : public torch::autograd::Function<RotaryNode> {
    static variable_list forward(AutogradContext* ctx, const at::Tensor& q_in, const at::Tensor& k_in, const at::Tensor& cos, const at::Tensor& sin,
                                 const c10::optional<at::Tensor>& pos, bool need) {
        const at::Tensor q = served(q_in), k = served(k_in);
        const int64_t B = q.size(0), T = q.size(2), D = q.size(3);
        const c10::ScalarType rdt = q.scalar_type() == k.scalar_type() ? q.scalar_type() : at::kFloat;      // ops.rope_result_dtype
        at::Tensor qo = dense_like(q.sizes(), q.strides(), q.options().dtype(rdt)), ko = dense_like(k.sizes(), k.strides(), k.options().dtype(rdt));
        const bool has_pos = pos.has_value() && pos->defined();
        const int64_t pbs = has_pos && pos->size(0) == B && B > 1 ? T : 0;
        {
            c10::DeviceGuard guard(q.device());
            void* stream = c10::hip::getCurrentHIPStream(q.device().index()).stream();
            const int rc = g_fwd(q.data_ptr(), k.data_ptr(), qo.data_ptr(), ko.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                 has_pos ? pos->data_ptr<int64_t>() : nullptr, pbs, B, q.size(1), k.size(1), T, D, cos.size(0), q.stride(0), q.stride(1),
                                 q.stride(2), k.stride(0), k.stride(1), k.stride(2), dtype_code(q.scalar_type()), dtype_code(k.scalar_type()),
                                 dtype_code(cos.scalar_type()), stream);
            TORCH_CHECK(rc == FQ_OK, "rope_forward failed (code ", rc, "): ", g_last_error ? g_last_error() : "");
            g_fwd_launch.fetch_add(1, std::memory_order_relaxed);
        }
        if (need) {                                       // no gradient can be asked for: nothing saved.  Neither q nor k ever is
            if (has_pos) ctx->save_for_backward({cos, sin, *pos});
            else ctx->save_for_backward({cos, sin});
            ctx->saved_data["q_sizes"] = q.sizes().vec();
            ctx->saved_data["q_strides"] = q.strides().vec();
            ctx->saved_data["k_sizes"] = k.sizes().vec();
            ctx->saved_data["k_strides"] = k.strides().vec();
            ctx->saved_data["q_dtype"] = (int64_t)q.scalar_type();
            ctx->saved_data["k_dtype"] = (int64_t)k.scalar_type();
        }
        return {qo, ko};
    }

    static variable_list backward(AutogradContext* ctx, variable_list grads) {
        const bool need_dq = ctx->needs_input_grad(0), need_dk = ctx->needs_input_grad(1);
        variable_list out(6);
        if (!(need_dq || need_dk)) return out;
        const auto saved = ctx->get_saved_variables();
        const at::Tensor &cos = saved[0], &sin = saved[1];
        const bool has_pos = saved.size() > 2;
        const std::vector<int64_t> qz = ctx->saved_data["q_sizes"].toIntVector(), qs = ctx->saved_data["q_strides"].toIntVector();
        const std::vector<int64_t> kz = ctx->saved_data["k_sizes"].toIntVector(), ks = ctx->saved_data["k_strides"].toIntVector();
        const int64_t B = qz[0], T = qz[2], D = qz[3];
        const auto qdt = (c10::ScalarType)ctx->saved_data["q_dtype"].toInt(), kdt = (c10::ScalarType)ctx->saved_data["k_dtype"].toInt();
        const at::TensorOptions opt = (need_dq ? grads[0] : grads[1]).options();      // the gradients: ops.rope_result_dtype
        at::Tensor gq, gk, dq, dk;                        // a frozen side: neither read, computed nor stored
        if (need_dq) {
            TORCH_CHECK(grads[0].defined() && grads[0].sizes() == c10::IntArrayRef(qz), "rope_backward: the gradient of q_embed has q's shape");
            gq = served(grads[0]);
            dq = dense_like(qz, qs, opt.dtype(qdt));
        }
        if (need_dk) {
            TORCH_CHECK(grads[1].defined() && grads[1].sizes() == c10::IntArrayRef(kz) && grads[1].options().dtype() == opt.dtype(),
                        "rope_backward: the gradient of k_embed has k's shape and dtype");
            gk = served(grads[1]);
            dk = dense_like(kz, ks, opt.dtype(kdt));
        }
        const int64_t pbs = has_pos && saved[2].size(0) == B && B > 1 ? T : 0;
        {
            c10::DeviceGuard guard(cos.device());
            void* stream = c10::hip::getCurrentHIPStream(cos.device().index()).stream();
            const int rc = g_bwd(need_dq ? gq.data_ptr() : nullptr, need_dk ? gk.data_ptr() : nullptr, need_dq ? dq.data_ptr() : nullptr,
                                 need_dk ? dk.data_ptr() : nullptr, cos.data_ptr(), sin.data_ptr(), has_pos ? saved[2].data_ptr<int64_t>() : nullptr, pbs, B,
                                 qz[1], kz[1], T, D, cos.size(0), need_dq ? gq.stride(0) : 0, need_dq ? gq.stride(1) : 0, need_dq ? gq.stride(2) : 0,
                                 need_dk ? gk.stride(0) : 0, need_dk ? gk.stride(1) : 0, need_dk ? gk.stride(2) : 0, qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],
                                 dtype_code(qdt), dtype_code(kdt), dtype_code(cos.scalar_type()), stream);
            TORCH_CHECK(rc == FQ_OK, "rope_backward failed (code ", rc, "): ", g_last_error ? g_last_error() : "");
            g_bwd_launch.fetch_add(1, std::memory_order_relaxed);
        }
        out[0] = dq;
        out[1] = dk;
        return out;
    }
};

void bind(uintptr_t fwd, uintptr_t bwd, uintptr_t dense, uintptr_t last_error) {
    g_fwd = reinterpret_cast<decltype(g_fwd)>(fwd);
    g_bwd = reinterpret_cast<decltype(g_bwd)>(bwd);
    g_dense = reinterpret_cast<decltype(g_dense)>(dense);
    g_last_error = reinterpret_cast<decltype(g_last_error)>(last_error);
}

std::vector<at::Tensor> rotary(const at::Tensor& q, const at::Tensor& k, const at::Tensor& cos, const at::Tensor& sin, const c10::optional<at::Tensor>& pos,
                               bool need) {
    TORCH_CHECK(g_fwd && g_bwd && g_dense, "the rotary node is not bound to the kernel library");
    return RotaryNode::apply(q, k, cos, sin, pos, need);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.attr("abi_version") = FQ_ABI_VERSION;
    m.def("bind", &bind);
    m.def("rotary", &rotary);
    m.def("counters", [] { return std::make_tuple(g_fwd_launch.load(), g_bwd_launch.load(), g_copy_route.load()); });
}
