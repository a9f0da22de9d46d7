// Host side of llm_qat_amd.mlp.swiglu as a C++ autograd node (PyTorch extension `_fq_act_node`, optional accelerator of mlp.py).
//
// What it replaces: mlp._SwiGLU (a Python torch.autograd.Function).  Why: the two kernels take 28 and 38 us on a bf16 [2048, 11008]
// pair and the eager chain they replace is GPU-bound from its first launch, so every microsecond of host work in front of a launch is
// added to the fused call's time; the Python Function put about 22 us there, forward and again backward (on the autograd engine's
// thread, under the GIL).  This node's forward is one allocation and one call through the C ABI, its backward two allocations and one.
//
// What it does not do: check arguments.  mlp.swiglu has run ops.check_swiglu (types, dtypes, shapes, devices, the CPU dispatch) and
// hands over (rows, cols); the layout rule is ops._act_rows restated (served_rows below).  The kernels are reached through the function
// pointers of the C ABI (include/llmqat_fakequant_act.h) that _act_node.py hands over: this file links against PyTorch, not against the
// HIP library.  Results are the Python node's bit for bit: the same entry points with the same arguments.
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <atomic>

#include "../../include/llmqat_fakequant_act.h"

namespace {

using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

decltype(&fqa_swiglu_fwd) g_fwd = nullptr;
decltype(&fqa_swiglu_bwd) g_bwd = nullptr;
decltype(&fq_last_error) g_last_error = nullptr;

// what ops.act_counts adds to its own counts
std::atomic<int64_t> g_fwd_launch{0}, g_bwd_launch{0}, g_copy_route{0};

inline int dtype_code(c10::ScalarType t) {
    return t == at::kFloat ? FQ_DTYPE_F32 : t == at::kBFloat16 ? FQ_DTYPE_BF16 : t == at::kHalf ? FQ_DTYPE_F16 : -1;
}

// ops._act_rows: a tensor is served where it lies when it is contiguous, or 2-D / 3-D with a last stride of 1, leading dimensions that
// collapse to one row stride, and that stride at least a row; anything else is copied once and counted -> the tensor to read, its stride
inline at::Tensor served_rows(const at::Tensor& t, int64_t cols, int64_t& stride) {
    if (t.is_contiguous()) {
        stride = cols;
        return t;
    }
    const int64_t nd = t.dim();
    if ((nd == 2 || nd == 3) && cols >= 2 && t.stride(nd - 1) == 1) {
        const int64_t s = t.stride(nd - 2);
        if (s >= cols && (nd == 2 || t.stride(0) == t.size(1) * s)) {
            stride = s;
            return t;
        }
    }
    g_copy_route.fetch_add(1, std::memory_order_relaxed);
    stride = cols;
    return t.contiguous();
}

struct SwiGluNode : public torch::autograd::Function<SwiGluNode> {
    static at::Tensor forward(AutogradContext* ctx, const at::Tensor& gate, const at::Tensor& up, int64_t rows, int64_t cols, bool need) {
        at::Tensor y = at::empty(gate.sizes(), gate.options());
        int64_t sg = cols, su = cols;
        at::Tensor g = gate, u = up;
        if (rows > 0) {
            g = served_rows(gate, cols, sg);
            u = served_rows(up, cols, su);
            c10::DeviceGuard guard(g.device());
            void* stream = c10::hip::getCurrentHIPStream(g.device().index()).stream();
            const int rc = g_fwd(g.data_ptr(), u.data_ptr(), y.data_ptr(), rows, cols, sg, su, dtype_code(g.scalar_type()), stream);
            TORCH_CHECK(rc == FQ_OK, "swiglu_forward failed (code ", rc, "): ", g_last_error ? g_last_error() : "");
            g_fwd_launch.fetch_add(1, std::memory_order_relaxed);
        }
        if (need) {                                       // no gradient can be asked for: nothing saved
            ctx->save_for_backward({g, u});
            ctx->saved_data["rows"] = rows;
            ctx->saved_data["cols"] = cols;
        }
        return y;
    }

    static variable_list backward(AutogradContext* ctx, variable_list grads) {
        const bool need_dgate = ctx->needs_input_grad(0), need_dup = ctx->needs_input_grad(1);
        variable_list out(5);
        if (!(need_dgate || need_dup)) return out;
        const auto saved = ctx->get_saved_variables();
        const at::Tensor &gate = saved[0], &up = saved[1];
        const at::Tensor& dy = grads[0];
        const int64_t rows = ctx->saved_data["rows"].toInt(), cols = ctx->saved_data["cols"].toInt();
        TORCH_CHECK(dy.defined() && dy.scalar_type() == gate.scalar_type() && dy.sizes() == gate.sizes() && dy.device() == gate.device(),
                    "swiglu_backward: dy is the gradient of y: the shape, dtype and device of gate");
        at::Tensor dgate = need_dgate ? at::empty(gate.sizes(), gate.options()) : at::Tensor();   // a frozen side: neither computed nor stored
        at::Tensor dup = need_dup ? at::empty(gate.sizes(), gate.options()) : at::Tensor();
        if (rows > 0) {
            int64_t sd = cols, sg = cols, su = cols;
            const at::Tensor d = served_rows(dy, cols, sd), g = served_rows(gate, cols, sg), u = served_rows(up, cols, su);
            c10::DeviceGuard guard(g.device());
            void* stream = c10::hip::getCurrentHIPStream(g.device().index()).stream();
            const int rc = g_bwd(d.data_ptr(), g.data_ptr(), u.data_ptr(), need_dgate ? dgate.data_ptr() : nullptr, need_dup ? dup.data_ptr() : nullptr,
                                 rows, cols, sd, sg, su, dtype_code(g.scalar_type()), stream);
            TORCH_CHECK(rc == FQ_OK, "swiglu_backward failed (code ", rc, "): ", g_last_error ? g_last_error() : "");
            g_bwd_launch.fetch_add(1, std::memory_order_relaxed);
        }
        out[0] = dgate;
        out[1] = dup;
        return out;
    }
};

void bind(uintptr_t fwd, uintptr_t bwd, uintptr_t last_error) {
    g_fwd = reinterpret_cast<decltype(g_fwd)>(fwd);
    g_bwd = reinterpret_cast<decltype(g_bwd)>(bwd);
    g_last_error = reinterpret_cast<decltype(g_last_error)>(last_error);
}

at::Tensor swiglu(const at::Tensor& gate, const at::Tensor& up, int64_t rows, int64_t cols, bool need) {
    TORCH_CHECK(g_fwd && g_bwd, "the SwiGLU node is not bound to the kernel library");
    return SwiGluNode::apply(gate, up, rows, cols, need);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.attr("abi_version") = FQ_ABI_VERSION;
    m.def("bind", &bind);
    m.def("swiglu", &swiglu);
    m.def("counters", [] { return std::make_tuple(g_fwd_launch.load(), g_bwd_launch.load(), g_copy_route.load()); });
}
