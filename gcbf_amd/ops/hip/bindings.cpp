// Python bindings for the gcbf_amd HIP/CDNA4 kernels (gfx950).
//
// Thin torch glue: tensor checks + allocation here, all device code in the
// .hip translation units (compiled with --offload-arch=gfx950).
#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

extern "C" void launch_seg_attn_fwd(const float* msg, const float* gate,
                                    const int* ptr, float* att, float* out,
                                    int N, int D, hipStream_t stream);
extern "C" void launch_seg_attn_bwd(const float* grad_out, const float* msg,
                                    const float* att, const int* ptr,
                                    float* dmsg, float* dgate, int N, int D,
                                    hipStream_t stream);
extern "C" void launch_seg_max_fwd(const float* values, const int* ptr,
                                   float* out, int* argmax, int N, int D,
                                   hipStream_t stream);
extern "C" void launch_seg_max_bwd(const float* grad_out, const int* argmax,
                                   float* dval, int N, int D,
                                   hipStream_t stream);
extern "C" void launch_radius_count(const float* pos, int* counts, int B,
                                    int N, int n_rec, int P, float r,
                                    int topk, hipStream_t stream);
extern "C" void launch_radius_fill(const float* pos, const float* states,
                                   const int* offsets, long* edge_index,
                                   float* edge_attr, long E_total, int B,
                                   int N, int n_rec, int P, int S, int A,
                                   float r, int topk, int attr_kind,
                                   hipStream_t stream);
extern "C" void launch_fused_linear_bf16(const void* A, const void* W,
                                         const float* bias, void* Cb,
                                         float* Cf, int M, int N, int K,
                                         int act, int out_f32,
                                         hipStream_t stream);
extern "C" void launch_pad_edges(const int* offsets, const int* counts,
                                 long* edge_index, long* seg,
                                 float* edge_attr, int* e_count, int rows,
                                 long E_max, long N_total, int A,
                                 hipStream_t stream);
extern "C" void launch_fused_masks(const float* states, bool* safe,
                                   bool* unsafe, bool* collision, int B,
                                   int N, int n_rec, int S, float r, int kind,
                                   hipStream_t stream);
extern "C" void launch_dubins_step(const float* states, const float* goal,
                                   const float* action, float* new_states,
                                   float* u_ref_next, float* reward,
                                   bool* reach, bool* collision, int N, int n,
                                   float dt, float r, float sl, float d2g,
                                   float act_lim, hipStream_t stream);
extern "C" void launch_car_step(const float* states, const float* goal,
                                const float* action, const float* K,
                                float* new_states, float* u_ref_next,
                                float* reward, bool* reach, bool* collision,
                                int N, float dt, float r, float sl, float d2g,
                                float act_lim, hipStream_t stream);
extern "C" void launch_drone_step(const float* states, const float* goal,
                                  const float* action, const float* K,
                                  float* new_states, float* u_ref_next,
                                  float* reward, bool* reach,
                                  bool* collision, int N, int n, float dt,
                                  float r, float sl, float d2g,
                                  float act_lim, hipStream_t stream);

extern "C" void launch_dubins_step_batched(
        const float* states, const float* goal, const float* action,
        const int* active, float* new_states, float* u_ref_next,
        float* reward, bool* reach, bool* collision, bool* reach_all, int B,
        int N, int n, float dt, float r, float sl, float d2g, float act_lim,
        hipStream_t stream);
extern "C" void launch_car_step_batched(
        const float* states, const float* goal, const float* action,
        const int* active, const float* K, float* new_states,
        float* u_ref_next, float* reward, bool* reach, bool* collision,
        bool* reach_all, int B, int N, float dt, float r, float sl,
        float d2g, float act_lim, hipStream_t stream);
extern "C" void launch_drone_step_batched(
        const float* states, const float* goal, const float* action,
        const int* active, const float* K, float* new_states,
        float* u_ref_next, float* reward, bool* reach, bool* collision,
        bool* reach_all, int B, int N, int n, float dt, float r, float sl,
        float d2g, float act_lim, hipStream_t stream);

extern "C" void launch_reset_sample(const float* cand, const float* min_sep,
                                    const float* avoid, float avoid_dist,
                                    float* pts, int* count, int* used, int B,
                                    int C, int A, int n, int dim,
                                    hipStream_t stream);

extern "C" int rollout_tail_max_rows();
extern "C" int rollout_tail_max_nodes();
extern "C" void launch_rollout_tail(
        int kind, const float* states_in, const float* goal,
        const float* action, const float* K, float* states_out,
        float* u_ref_next, float* reward, bool* reach, bool* collision,
        long* edge_index, long* seg, float* edge_attr, int* flags, int N,
        int n, int n_rec, int S, int P, float dt, float r_agent, float sl,
        float d2g, float act_lim, float r_comm, int attr_kind, int A_attr,
        long E_max, int topk, int threads, hipStream_t stream);

extern "C" int rollout_tail_batched_max_rows();
extern "C" int rollout_tail_batched_max_nodes();
extern "C" int rollout_tail_batched_max_scenes();
extern "C" void launch_rollout_tail_batched(
        int kind, const float* states_in, const float* goal,
        const float* action, const int* explore, const float* K,
        float* states_out, float* u_ref_next, float* reward, bool* reach,
        bool* collision, int* counts, float* thr, long* edge_index, long* seg,
        float* edge_attr, int* flags, int* e_count, int B, int N, int n,
        int n_rec, int S, int G, int A, int P, float dt, float r_agent,
        float sl, float d2g, float act_lim, float r_comm, int attr_kind,
        int A_attr, long E_cap, int topk, int threads, hipStream_t stream);

extern "C" void launch_edge_inputs_bf16(const float* x, const long* ei,
                                        const float* ea, void* out, int N,
                                        int nd, int ed, long E, long rows,
                                        hipStream_t stream);
extern "C" void launch_attn_gamma_in(const void* msg, const void* gate,
                                     int gate_is_bf16, const long* seg,
                                     const float* x, const long* idx,
                                     float* att, void* out, int E, int D,
                                     int nd, int n_rows, int num_nodes,
                                     int rows, hipStream_t stream);
extern "C" void launch_edge_inputs_bwd(const void* din, float* dea, int nd,
                                       int ed, long E, hipStream_t stream);
extern "C" void launch_attn_gamma_in_bwd_gate(
        const void* dout, const void* msg, const float* att, const long* seg,
        const long* idx, float* stage, void* dgate, int E, int D, int nd,
        int n_rows, int num_nodes, int rows, hipStream_t stream);
extern "C" void launch_attn_gamma_in_bwd_msg(
        const void* dout, const float* att, const long* seg, const long* idx,
        const void* dmsg_gate, void* dmsg, int E, int D, int nd, int n_rows,
        int num_nodes, int rows, int round_prod, hipStream_t stream);
extern "C" void launch_rows_cat_bwd(const void* din, void* da, int Da, int Db,
                                    long n_rows, long rows,
                                    hipStream_t stream);
extern "C" void launch_rows_cat_pad_bf16(const void* a, const float* b,
                                         void* out, int Da, int Db,
                                         long n_rows, long rows,
                                         hipStream_t stream);
extern "C" void launch_refresh_mirrors(const long long* table, int n_layers,
                                       long max_groups, hipStream_t stream);
extern "C" void launch_segmax_rows_bf16(const void* msg, const long* seg,
                                        const long* idx, void* out, int E,
                                        int D, int n_rows, int num_nodes,
                                        int rows, hipStream_t stream);

namespace {

#define CHECK_IN(x)                                                   \
    TORCH_CHECK(x.is_cuda(), #x " must be on GPU");                    \
    TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

hipStream_t current_stream() {
    return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

std::vector<torch::Tensor> segment_attn_fwd(torch::Tensor msg,
                                            torch::Tensor gate,
                                            torch::Tensor ptr) {
    CHECK_IN(msg);
    CHECK_IN(gate);
    CHECK_IN(ptr);
    TORCH_CHECK(msg.scalar_type() == torch::kFloat32, "msg must be fp32");
    TORCH_CHECK(ptr.scalar_type() == torch::kInt32, "ptr must be int32");
    const int64_t E = msg.size(0), D = msg.size(1);
    const int64_t N = ptr.size(0) - 1;
    // att is zero-initialized for the same reason as the backward outputs:
    // edges past the last CSR segment (sentinel pads) are never written by
    // the kernel and must not surface uninitialized memory
    auto att = torch::zeros({E}, msg.options());
    auto out = torch::empty({N, D}, msg.options());
    if (N > 0)
        launch_seg_attn_fwd(msg.data_ptr<float>(), gate.data_ptr<float>(),
                            ptr.data_ptr<int>(), att.data_ptr<float>(),
                            out.data_ptr<float>(), (int)N, (int)D,
                            current_stream());
    return {att, out};
}

std::vector<torch::Tensor> segment_attn_bwd(torch::Tensor grad_out,
                                            torch::Tensor msg,
                                            torch::Tensor att,
                                            torch::Tensor ptr) {
    CHECK_IN(grad_out);
    CHECK_IN(msg);
    CHECK_IN(att);
    CHECK_IN(ptr);
    const int64_t E = msg.size(0), D = msg.size(1);
    const int64_t N = ptr.size(0) - 1;
    // zeros, not empty: the kernel only writes edges covered by a CSR
    // segment, and padded edge buffers (sentinel segment id past the last
    // node) legitimately contain uncovered edges — leaving those rows
    // uninitialized poisoned every gradient downstream of the aggregation
    // in the captured update engine
    auto dmsg = torch::zeros_like(msg);
    auto dgate = torch::zeros({E}, msg.options());
    if (N > 0)
        launch_seg_attn_bwd(grad_out.data_ptr<float>(), msg.data_ptr<float>(),
                            att.data_ptr<float>(), ptr.data_ptr<int>(),
                            dmsg.data_ptr<float>(), dgate.data_ptr<float>(),
                            (int)N, (int)D, current_stream());
    return {dmsg, dgate};
}

std::vector<torch::Tensor> segment_max_fwd(torch::Tensor values,
                                           torch::Tensor ptr) {
    CHECK_IN(values);
    CHECK_IN(ptr);
    const int64_t D = values.size(1);
    const int64_t N = ptr.size(0) - 1;
    auto out = torch::empty({N, D}, values.options());
    auto argmax = torch::empty({N, D},
                               values.options().dtype(torch::kInt32));
    if (N > 0)
        launch_seg_max_fwd(values.data_ptr<float>(), ptr.data_ptr<int>(),
                           out.data_ptr<float>(), argmax.data_ptr<int>(),
                           (int)N, (int)D, current_stream());
    return {out, argmax};
}

torch::Tensor segment_max_bwd(torch::Tensor grad_out, torch::Tensor argmax,
                              int64_t E) {
    CHECK_IN(grad_out);
    CHECK_IN(argmax);
    const int64_t N = grad_out.size(0), D = grad_out.size(1);
    auto dval = torch::zeros({E, D}, grad_out.options());
    if (N > 0)
        launch_seg_max_bwd(grad_out.data_ptr<float>(),
                           argmax.data_ptr<int>(), dval.data_ptr<float>(),
                           (int)N, (int)D, current_stream());
    return dval;
}

// Argument checks shared by build_graph and build_graph_padded; every one
// fires before the first launch.  Returns N, the nodes per graph.
static int64_t check_graph_args(const torch::Tensor& pos,
                                const torch::Tensor& states, int64_t B,
                                int64_t n_rec, int64_t attr_kind,
                                int64_t attr_dim) {
    CHECK_IN(pos);
    CHECK_IN(states);
    TORCH_CHECK(pos.scalar_type() == torch::kFloat32, "pos must be fp32");
    TORCH_CHECK(states.scalar_type() == torch::kFloat32,
                "states must be fp32");
    TORCH_CHECK(pos.dim() == 2 && states.dim() == 2,
                "pos and states must be 2-D");
    TORCH_CHECK(pos.device() == states.device(),
                "pos and states must share a device");
    TORCH_CHECK(B >= 1, "B must be >= 1 (got ", B, ")");
    TORCH_CHECK(pos.size(0) % B == 0, "pos rows (", pos.size(0),
                ") must be a multiple of B (", B, ")");
    TORCH_CHECK(states.size(0) == pos.size(0), "states rows (",
                states.size(0), ") != pos rows (", pos.size(0), ")");
    const int64_t N = pos.size(0) / B;
    const int64_t P = pos.size(1), S = states.size(1);
    TORCH_CHECK(P >= 1 && P <= S, "need 1 <= P <= S (got P=", P, ", S=", S,
                ")");
    TORCH_CHECK(n_rec >= 0 && n_rec <= N, "need 0 <= n_rec <= N (got n_rec=",
                n_rec, ", N=", N, ")");
    TORCH_CHECK(attr_kind == 0 || attr_kind == 1,
                "attr_kind must be 0 (diff) or 1 (dubins), got ", attr_kind);
    if (attr_kind == 0) {
        TORCH_CHECK(attr_dim == S, "ATTR_DIFF needs attr_dim == S (got ",
                    attr_dim, " vs ", S, ")");
    } else {
        TORCH_CHECK(S == 4 && attr_dim == 5,
                    "ATTR_DUBINS needs S == 4 and attr_dim == 5 (got S=", S,
                    ", attr_dim=", attr_dim, ")");
    }
    return N;
}

std::vector<torch::Tensor> build_graph(torch::Tensor pos,
                                       torch::Tensor states, int64_t B,
                                       int64_t n_rec, double r, int64_t topk,
                                       int64_t attr_kind, int64_t attr_dim) {
    const int64_t N = check_graph_args(pos, states, B, n_rec, attr_kind,
                                       attr_dim);
    const int64_t P = pos.size(1), S = states.size(1);
    if (B * n_rec == 0)  // no receiver rows: nothing to launch
        return {torch::empty({2, 0}, pos.options().dtype(torch::kInt64)),
                torch::empty({0, attr_dim}, pos.options())};
    auto stream = current_stream();
    auto counts = torch::empty({B * n_rec},
                               pos.options().dtype(torch::kInt32));
    launch_radius_count(pos.data_ptr<float>(), counts.data_ptr<int>(),
                        (int)B, (int)N, (int)n_rec, (int)P, (float)r,
                        (int)topk, stream);
    auto incl = counts.cumsum(0, torch::kInt32);
    auto offsets = (incl - counts).contiguous();
    const int64_t E = incl[-1].item<int64_t>();
    auto edge_index = torch::empty({2, E},
                                   pos.options().dtype(torch::kInt64));
    auto edge_attr = torch::empty({E, attr_dim}, pos.options());
    if (E > 0)
        launch_radius_fill(pos.data_ptr<float>(), states.data_ptr<float>(),
                           offsets.data_ptr<int>(),
                           edge_index.data_ptr<int64_t>(),
                           edge_attr.data_ptr<float>(), E, (int)B, (int)N,
                           (int)n_rec, (int)P, (int)S, (int)attr_dim,
                           (float)r, (int)topk, (int)attr_kind, stream);
    return {edge_index, edge_attr};
}

std::vector<torch::Tensor> fused_masks(torch::Tensor states, int64_t B,
                                       int64_t n_rec, double r, int64_t kind,
                                       bool want_safe, bool want_unsafe,
                                       bool want_coll) {
    CHECK_IN(states);
    const int64_t N = states.size(0) / B;
    const int64_t S = states.size(1);
    auto opts = states.options().dtype(torch::kBool);
    auto none = torch::Tensor();
    auto t_safe = want_safe ? torch::empty({B * n_rec}, opts) : none;
    auto t_uns = want_unsafe ? torch::empty({B * n_rec}, opts) : none;
    auto t_coll = want_coll ? torch::empty({B * n_rec}, opts) : none;
    launch_fused_masks(
        states.data_ptr<float>(),
        want_safe ? t_safe.data_ptr<bool>() : nullptr,
        want_unsafe ? t_uns.data_ptr<bool>() : nullptr,
        want_coll ? t_coll.data_ptr<bool>() : nullptr,
        (int)B, (int)N, (int)n_rec, (int)S, (float)r, (int)kind,
        current_stream());
    return {t_safe, t_uns, t_coll};
}

std::vector<torch::Tensor> build_graph_padded(
        torch::Tensor pos, torch::Tensor states, int64_t B, int64_t n_rec,
        double r, int64_t topk, int64_t attr_kind, int64_t attr_dim,
        int64_t E_max,
        c10::optional<std::vector<torch::Tensor>> out_opt = c10::nullopt) {
    // capture-safe variant: fixed E_max edge buffers, no host sync.
    const int64_t N = check_graph_args(pos, states, B, n_rec, attr_kind,
                                       attr_dim);
    TORCH_CHECK(E_max >= 0, "E_max must be >= 0 (got ", E_max, ")");
    const int64_t P = pos.size(1), S = states.size(1);
    torch::Tensor edge_index, seg, edge_attr, e_count;
    if (out_opt.has_value()) {
        TORCH_CHECK(out_opt->size() == 4,
                    "out must be {edge_index, seg, edge_attr, e_count}");
        for (const auto& t : *out_opt) { CHECK_IN(t); }
        edge_index = (*out_opt)[0];
        seg = (*out_opt)[1];
        edge_attr = (*out_opt)[2];
        e_count = (*out_opt)[3];
        TORCH_CHECK(edge_index.scalar_type() == torch::kInt64
                    && seg.scalar_type() == torch::kInt64,
                    "out edge_index and seg must be int64");
        TORCH_CHECK(edge_attr.scalar_type() == torch::kFloat32,
                    "out edge_attr must be fp32");
        TORCH_CHECK(e_count.scalar_type() == torch::kInt32,
                    "out e_count must be int32");
        TORCH_CHECK(edge_index.dim() == 2 && edge_index.size(0) == 2
                    && seg.dim() == 1 && edge_attr.dim() == 2,
                    "out must be edge_index (2, E_max), seg (E_max,), "
                    "edge_attr (E_max, attr_dim)");
        TORCH_CHECK(edge_index.size(1) == E_max && seg.size(0) == E_max
                    && edge_attr.size(0) == E_max, "E_max mismatch");
        TORCH_CHECK(edge_attr.size(1) == attr_dim, "out edge_attr has ",
                    edge_attr.size(1), " columns, attr_dim is ", attr_dim);
        TORCH_CHECK(e_count.numel() == 1, "out e_count must hold 1 element");
    } else {
        edge_index = torch::empty({2, E_max},
                                  pos.options().dtype(torch::kInt64));
        seg = torch::empty({E_max}, pos.options().dtype(torch::kInt64));
        edge_attr = torch::empty({E_max, attr_dim}, pos.options());
        e_count = torch::empty({1}, pos.options().dtype(torch::kInt32));
    }
    if (B * n_rec == 0) {
        // no receiver rows: every entry is a pad, nothing to launch
        edge_index.zero_();
        seg.fill_(B * N);
        edge_attr.zero_();
        e_count.zero_();
        return {edge_index, seg, edge_attr, e_count};
    }
    auto stream = current_stream();
    auto counts = torch::empty({B * n_rec},
                               pos.options().dtype(torch::kInt32));
    launch_radius_count(pos.data_ptr<float>(), counts.data_ptr<int>(),
                        (int)B, (int)N, (int)n_rec, (int)P, (float)r,
                        (int)topk, stream);
    auto incl = counts.cumsum(0, torch::kInt32);
    auto offsets = (incl - counts).contiguous();
    launch_radius_fill(pos.data_ptr<float>(), states.data_ptr<float>(),
                       offsets.data_ptr<int>(),
                       edge_index.data_ptr<int64_t>(),
                       edge_attr.data_ptr<float>(), E_max, (int)B, (int)N,
                       (int)n_rec, (int)P, (int)S, (int)attr_dim, (float)r,
                       (int)topk, (int)attr_kind, stream);
    launch_pad_edges(offsets.data_ptr<int>(), counts.data_ptr<int>(),
                     edge_index.data_ptr<int64_t>(),
                     seg.data_ptr<int64_t>(), edge_attr.data_ptr<float>(),
                     e_count.data_ptr<int>(), (int)(B * n_rec), E_max,
                     B * N, (int)attr_dim, stream);
    return {edge_index, seg, edge_attr, e_count};
}

torch::Tensor fused_linear(torch::Tensor x, torch::Tensor w,
                           c10::optional<torch::Tensor> bias, int64_t act,
                           bool out_f32) {
    CHECK_IN(x);
    CHECK_IN(w);
    TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "x must be bf16");
    TORCH_CHECK(w.scalar_type() == torch::kBFloat16, "w must be bf16");
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "x and w must be 2-D");
    const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
    TORCH_CHECK(w.size(1) == K, "K mismatch");
    TORCH_CHECK(M % 128 == 0 && N % 128 == 0 && K % 64 == 0,
                "fused_linear needs M%128==0, N%128==0, K%64==0 (got ", M,
                "x", K, " -> ", N, ")");
    TORCH_CHECK(M > 0 && N > 0 && K > 0,
                "fused_linear needs M, N, K > 0 (got ", M, "x", K, " -> ", N,
                ")");
    TORCH_CHECK(act >= 0 && act <= 2,
                "act must be 0 (none), 1 (relu) or 2 (tanh), got ", act);
    const float* bptr = nullptr;
    if (bias.has_value()) {
        CHECK_IN(bias.value());
        TORCH_CHECK(bias->scalar_type() == torch::kFloat32,
                    "bias must be fp32");
        TORCH_CHECK(bias->numel() == N, "bias has ", bias->numel(),
                    " elements, N is ", N);
        bptr = bias->data_ptr<float>();
    }
    auto out = torch::empty({M, N}, x.options().dtype(
        out_f32 ? torch::kFloat32 : torch::kBFloat16));
    launch_fused_linear_bf16(
        x.data_ptr(), w.data_ptr(), bptr,
        out_f32 ? nullptr : out.data_ptr(),
        out_f32 ? out.data_ptr<float>() : nullptr,
        (int)M, (int)N, (int)K, (int)act, out_f32 ? 1 : 0,
        current_stream());
    return out;
}

struct StepOut {
    torch::Tensor new_states, u_ref_next, reward, reach, collision;
};

static std::vector<torch::Tensor> alloc_step_out(
        torch::Tensor states, int64_t n, int64_t A,
        const c10::optional<std::vector<torch::Tensor>>& out) {
    if (out.has_value()) {
        // caller-provided output buffers (ping-pong rollout capture: the
        // kernels write the next phase's inputs directly, no copy-back)
        TORCH_CHECK(out->size() == 5, "out must be "
                    "{new_states, u_ref_next, reward, reach, collision}");
        for (const auto& t : *out) { CHECK_IN(t); }
        return *out;
    }
    auto f = states.options();
    auto b = states.options().dtype(torch::kBool);
    return {torch::empty_like(states), torch::empty({n, A}, f),
            torch::empty({n}, f), torch::empty({n}, b),
            torch::empty({n}, b)};
}

std::vector<torch::Tensor> dubins_step(
        torch::Tensor states, torch::Tensor goal, torch::Tensor action,
        double dt, double r, double sl, double d2g, double act_lim,
        c10::optional<std::vector<torch::Tensor>> out_opt = c10::nullopt) {
    CHECK_IN(states); CHECK_IN(goal); CHECK_IN(action);
    const int64_t N = states.size(0), n = action.size(0);
    auto out = alloc_step_out(states, n, 2, out_opt);
    launch_dubins_step(states.data_ptr<float>(), goal.data_ptr<float>(),
                       action.data_ptr<float>(), out[0].data_ptr<float>(),
                       out[1].data_ptr<float>(), out[2].data_ptr<float>(),
                       out[3].data_ptr<bool>(), out[4].data_ptr<bool>(),
                       (int)N, (int)n, (float)dt, (float)r, (float)sl,
                       (float)d2g, (float)act_lim, current_stream());
    return out;
}

std::vector<torch::Tensor> car_step(
        torch::Tensor states, torch::Tensor goal, torch::Tensor action,
        torch::Tensor K, double dt, double r, double sl, double d2g,
        double act_lim,
        c10::optional<std::vector<torch::Tensor>> out_opt = c10::nullopt) {
    CHECK_IN(states); CHECK_IN(goal); CHECK_IN(action); CHECK_IN(K);
    const int64_t N = states.size(0);
    auto out = alloc_step_out(states, N, 2, out_opt);
    launch_car_step(states.data_ptr<float>(), goal.data_ptr<float>(),
                    action.data_ptr<float>(), K.data_ptr<float>(),
                    out[0].data_ptr<float>(), out[1].data_ptr<float>(),
                    out[2].data_ptr<float>(), out[3].data_ptr<bool>(),
                    out[4].data_ptr<bool>(), (int)N, (float)dt, (float)r,
                    (float)sl, (float)d2g, (float)act_lim, current_stream());
    return out;
}

std::vector<torch::Tensor> drone_step(
        torch::Tensor states, torch::Tensor goal, torch::Tensor action,
        torch::Tensor K, double dt, double r, double sl, double d2g,
        double act_lim,
        c10::optional<std::vector<torch::Tensor>> out_opt = c10::nullopt) {
    CHECK_IN(states); CHECK_IN(goal); CHECK_IN(action); CHECK_IN(K);
    const int64_t N = states.size(0), n = action.size(0);
    auto out = alloc_step_out(states, n, 3, out_opt);
    launch_drone_step(states.data_ptr<float>(), goal.data_ptr<float>(),
                      action.data_ptr<float>(), K.data_ptr<float>(),
                      out[0].data_ptr<float>(), out[1].data_ptr<float>(),
                      out[2].data_ptr<float>(), out[3].data_ptr<bool>(),
                      out[4].data_ptr<bool>(), (int)N, (int)n, (float)dt,
                      (float)r, (float)sl, (float)d2g, (float)act_lim,
                      current_stream());
    return out;
}

// ---- batched step (env_step_batched.hip): B scenes of identical shape
#define CHECK_F32(x, ...)                                              \
    CHECK_IN(x);                                                       \
    TORCH_CHECK(x.scalar_type() == torch::kFloat32, #x " must be fp32"); \
    TORCH_CHECK(x.sizes() == torch::IntArrayRef({__VA_ARGS__}),        \
                #x " has shape ", x.sizes(), ", expected {" #__VA_ARGS__ "}")
#define CHECK_BOOL(x, ...)                                             \
    CHECK_IN(x);                                                       \
    TORCH_CHECK(x.scalar_type() == torch::kBool, #x " must be bool");  \
    TORCH_CHECK(x.sizes() == torch::IntArrayRef({__VA_ARGS__}),        \
                #x " has shape ", x.sizes(), ", expected {" #__VA_ARGS__ "}")

// checks the inputs every batched step shares and returns the six output
// buffers {new_states, u_ref_next, reward, reach, collision, reach_all}
static std::vector<torch::Tensor> batched_step_io(
        const torch::Tensor& states, const torch::Tensor& goal,
        const torch::Tensor& action, const torch::Tensor& active, int64_t S,
        int64_t G, int64_t A,
        const c10::optional<std::vector<torch::Tensor>>& out_opt) {
    TORCH_CHECK(states.dim() == 3 && action.dim() == 3,
                "states (B, N, S) and action (B, n, A) expected");
    const int64_t B = states.size(0), N = states.size(1),
                  n = action.size(1);
    TORCH_CHECK(n >= 1 && n <= N, "need 1 <= n <= N, got n=", n, " N=", N);
    TORCH_CHECK(B <= 65535, "at most 65535 scenes per launch, got ", B);
    TORCH_CHECK(N * S < (int64_t(1) << 31), "scene too large");
    CHECK_F32(states, B, N, S);
    CHECK_F32(goal, B, n, G);
    CHECK_F32(action, B, n, A);
    CHECK_IN(active);
    TORCH_CHECK(active.scalar_type() == torch::kInt32 &&
                active.dim() == 1 && active.size(0) == B,
                "active must be int32 of shape (B,)");
    if (out_opt.has_value()) {
        TORCH_CHECK(out_opt->size() == 6, "out must be {new_states, "
                    "u_ref_next, reward, reach, collision, reach_all}");
        const auto& new_states = (*out_opt)[0];
        const auto& u_ref_next = (*out_opt)[1];
        const auto& reward = (*out_opt)[2];
        const auto& reach = (*out_opt)[3];
        const auto& collision = (*out_opt)[4];
        const auto& reach_all = (*out_opt)[5];
        CHECK_F32(new_states, B, N, S);
        CHECK_F32(u_ref_next, B, n, A);
        CHECK_F32(reward, B, n);
        CHECK_BOOL(reach, B, n);
        CHECK_BOOL(collision, B, n);
        CHECK_BOOL(reach_all, B);
        TORCH_CHECK(new_states.data_ptr() != states.data_ptr(),
                    "new_states must not alias states");
        return *out_opt;
    }
    auto f = states.options();
    auto b = states.options().dtype(torch::kBool);
    return {torch::empty_like(states), torch::empty({B, n, A}, f),
            torch::empty({B, n}, f), torch::empty({B, n}, b),
            torch::empty({B, n}, b), torch::empty({B}, b)};
}

std::vector<torch::Tensor> dubins_step_batched(
        torch::Tensor states, torch::Tensor goal, torch::Tensor action,
        torch::Tensor active, double dt, double r, double sl, double d2g,
        double act_lim,
        c10::optional<std::vector<torch::Tensor>> out_opt = c10::nullopt) {
    auto out = batched_step_io(states, goal, action, active, 4, 4, 2,
                               out_opt);
    const int64_t B = states.size(0);
    if (B > 0)
        launch_dubins_step_batched(
            states.data_ptr<float>(), goal.data_ptr<float>(),
            action.data_ptr<float>(), active.data_ptr<int>(),
            out[0].data_ptr<float>(), out[1].data_ptr<float>(),
            out[2].data_ptr<float>(), out[3].data_ptr<bool>(),
            out[4].data_ptr<bool>(), out[5].data_ptr<bool>(), (int)B,
            (int)states.size(1), (int)action.size(1), (float)dt, (float)r,
            (float)sl, (float)d2g, (float)act_lim, current_stream());
    return out;
}

std::vector<torch::Tensor> car_step_batched(
        torch::Tensor states, torch::Tensor goal, torch::Tensor action,
        torch::Tensor active, torch::Tensor K, double dt, double r,
        double sl, double d2g, double act_lim,
        c10::optional<std::vector<torch::Tensor>> out_opt = c10::nullopt) {
    auto out = batched_step_io(states, goal, action, active, 4, 2, 2,
                               out_opt);
    const int64_t B = states.size(0);
    TORCH_CHECK(states.size(1) == action.size(1),
                "SimpleCar has no obstacle rows: N must equal n");
    CHECK_F32(K, 2, 4);
    if (B > 0)
        launch_car_step_batched(
            states.data_ptr<float>(), goal.data_ptr<float>(),
            action.data_ptr<float>(), active.data_ptr<int>(),
            K.data_ptr<float>(), out[0].data_ptr<float>(),
            out[1].data_ptr<float>(), out[2].data_ptr<float>(),
            out[3].data_ptr<bool>(), out[4].data_ptr<bool>(),
            out[5].data_ptr<bool>(), (int)B, (int)states.size(1), (float)dt,
            (float)r, (float)sl, (float)d2g, (float)act_lim,
            current_stream());
    return out;
}

std::vector<torch::Tensor> drone_step_batched(
        torch::Tensor states, torch::Tensor goal, torch::Tensor action,
        torch::Tensor active, torch::Tensor K, double dt, double r,
        double sl, double d2g, double act_lim,
        c10::optional<std::vector<torch::Tensor>> out_opt = c10::nullopt) {
    auto out = batched_step_io(states, goal, action, active, 6, 6, 3,
                               out_opt);
    const int64_t B = states.size(0);
    CHECK_F32(K, 3, 6);
    if (B > 0)
        launch_drone_step_batched(
            states.data_ptr<float>(), goal.data_ptr<float>(),
            action.data_ptr<float>(), active.data_ptr<int>(),
            K.data_ptr<float>(), out[0].data_ptr<float>(),
            out[1].data_ptr<float>(), out[2].data_ptr<float>(),
            out[3].data_ptr<bool>(), out[4].data_ptr<bool>(),
            out[5].data_ptr<bool>(), (int)B, (int)states.size(1),
            (int)action.size(1), (float)dt, (float)r, (float)sl, (float)d2g,
            (float)act_lim, current_stream());
    return out;
}

torch::Tensor reset_sample(torch::Tensor cand, torch::Tensor min_sep,
                           torch::Tensor avoid, double avoid_dist,
                           torch::Tensor pts, torch::Tensor count) {
    // greedy rejection sampling over a candidate pool, one wave per problem;
    // pts/count are updated in place (resumable), returns used (B,) int32
    CHECK_IN(cand); CHECK_IN(min_sep); CHECK_IN(avoid);
    CHECK_IN(pts); CHECK_IN(count);
    TORCH_CHECK(cand.scalar_type() == torch::kFloat32 &&
                min_sep.scalar_type() == torch::kFloat32 &&
                avoid.scalar_type() == torch::kFloat32 &&
                pts.scalar_type() == torch::kFloat32,
                "cand, min_sep, avoid, pts must be fp32");
    TORCH_CHECK(count.scalar_type() == torch::kInt32, "count must be int32");
    TORCH_CHECK(cand.dim() == 3 && avoid.dim() == 3 && pts.dim() == 3,
                "cand (B,C,dim), avoid (B,A,dim), pts (B,n,dim) expected");
    const int64_t B = cand.size(0), C = cand.size(1), dim = cand.size(2);
    const int64_t A = avoid.size(1), n = pts.size(1);
    TORCH_CHECK(dim == 2 || dim == 3, "dim must be 2 or 3");
    TORCH_CHECK(avoid.size(0) == B && avoid.size(2) == dim &&
                pts.size(0) == B && pts.size(2) == dim &&
                min_sep.numel() == B && count.numel() == B,
                "reset_sample: batch/dim mismatch");
    // accepted points are kept in LDS: n*dim floats (48 KiB at the cap)
    TORCH_CHECK(n >= 0 && n <= 4096, "reset_sample: n must be <= 4096 "
                "(LDS budget), got ", n);
    TORCH_CHECK(C < (1 << 30) && A < (1 << 30), "pool too large");
    auto used = torch::zeros({B}, count.options());
    if (B > 0)
        launch_reset_sample(cand.data_ptr<float>(),
                            min_sep.data_ptr<float>(),
                            avoid.data_ptr<float>(), (float)avoid_dist,
                            pts.data_ptr<float>(), count.data_ptr<int>(),
                            used.data_ptr<int>(), (int)B, (int)C, (int)A,
                            (int)n, (int)dim, current_stream());
    return used;
}

// ---- rollout tail (rollout_tail.hip): mask -> step -> graph rebuild ->
// flags of one scene in one single-workgroup launch
std::vector<int64_t> rollout_tail_bounds() {
    return {rollout_tail_max_rows(), rollout_tail_max_nodes()};
}

void rollout_tail(int64_t kind, torch::Tensor states, torch::Tensor goal,
                  torch::Tensor action, c10::optional<torch::Tensor> K,
                  double dt, double r, double sl, double d2g, double act_lim,
                  int64_t n_rec, double comm_radius, int64_t attr_kind,
                  int64_t attr_dim, int64_t E_max,
                  std::vector<torch::Tensor> out, int64_t threads,
                  int64_t topk) {
    // kinds as in masks.hip: 0 car, 1 dubins, 2 drone
    TORCH_CHECK(kind >= 0 && kind <= 2, "rollout_tail: unknown env kind ",
                kind);
    TORCH_CHECK(topk == -1 || (topk >= 1 && topk < (int64_t(1) << 31)),
                "rollout_tail: topk must be -1 (no cap) or >= 1, got ", topk);
    const int64_t S = kind == 2 ? 6 : 4, P = kind == 2 ? 3 : 2;
    const int64_t A = kind == 2 ? 3 : 2, G = kind == 0 ? 2 : S;
    TORCH_CHECK(states.dim() == 2 && action.dim() == 2,
                "rollout_tail: states (N, S) and action (n, A) expected");
    const int64_t N = states.size(0), n = action.size(0);
    CHECK_F32(states, N, S);
    CHECK_F32(goal, n, G);
    CHECK_F32(action, n, A);
    TORCH_CHECK(n >= 1 && n <= N && (kind != 0 || n == N),
                "rollout_tail: bad agent count ", n, " for ", N, " nodes");
    const float* kptr = nullptr;
    if (kind != 1) {
        TORCH_CHECK(K.has_value(), "rollout_tail: this env needs the gain K");
        const torch::Tensor& Kt = K.value();
        CHECK_F32(Kt, A, S);
        kptr = Kt.data_ptr<float>();
    }
    TORCH_CHECK(n_rec >= 1 && n_rec <= n,
                "rollout_tail: n_rec must be in [1, n]");
    TORCH_CHECK(n_rec <= rollout_tail_max_rows() &&
                N <= rollout_tail_max_nodes(),
                "rollout_tail: scene (", n_rec, " receivers, ", N,
                " nodes) above the single-workgroup bound (",
                rollout_tail_max_rows(), ", ", rollout_tail_max_nodes(), ")");
    TORCH_CHECK((attr_kind == 0 && attr_dim == S) ||
                (attr_kind == 1 && S == 4 && attr_dim == 5),
                "rollout_tail: attr_kind/attr_dim mismatch");
    TORCH_CHECK(E_max >= 0 && E_max <= n_rec * (N - 1) + 64,
                "rollout_tail: bad E_max ", E_max);
    TORCH_CHECK(threads == 256 || threads == 512 || threads == 1024,
                "rollout_tail: threads must be 256, 512 or 1024");
    TORCH_CHECK(out.size() == 9, "out must be {new_states, u_ref_next, "
                "reward, reach, collision, edge_index, seg, edge_attr, "
                "flags}");
    const torch::Tensor &new_states = out[0], &u_ref_next = out[1],
        &reward = out[2], &reach = out[3], &collision = out[4],
        &edge_index = out[5], &seg = out[6], &edge_attr = out[7],
        &flags = out[8];
    CHECK_F32(new_states, N, S);
    CHECK_F32(u_ref_next, n, A);
    CHECK_F32(reward, n);
    CHECK_BOOL(reach, n);
    CHECK_BOOL(collision, n);
    CHECK_F32(edge_attr, E_max, attr_dim);
    CHECK_IN(edge_index); CHECK_IN(seg); CHECK_IN(flags);
    TORCH_CHECK(edge_index.scalar_type() == torch::kInt64 &&
                seg.scalar_type() == torch::kInt64 &&
                edge_index.sizes() == torch::IntArrayRef({2, E_max}) &&
                seg.sizes() == torch::IntArrayRef({E_max}),
                "rollout_tail: edge_index (2, E_max) / seg (E_max,) int64 "
                "expected");
    TORCH_CHECK(flags.scalar_type() == torch::kInt32 && flags.numel() == 3,
                "rollout_tail: flags must be int32 (3,)");
    TORCH_CHECK(new_states.data_ptr() != states.data_ptr(),
                "rollout_tail: new_states must not alias states");
    launch_rollout_tail(
        (int)kind, states.data_ptr<float>(), goal.data_ptr<float>(),
        action.data_ptr<float>(), kptr, new_states.data_ptr<float>(),
        u_ref_next.data_ptr<float>(), reward.data_ptr<float>(),
        reach.data_ptr<bool>(), collision.data_ptr<bool>(),
        edge_index.data_ptr<int64_t>(), seg.data_ptr<int64_t>(),
        edge_attr.data_ptr<float>(), flags.data_ptr<int>(), (int)N, (int)n,
        (int)n_rec, (int)S, (int)P, (float)dt, (float)r, (float)sl,
        (float)d2g, (float)act_lim, (float)comm_radius, (int)attr_kind,
        (int)attr_dim, E_max, (int)topk, (int)threads, current_stream());
}

// ---- batched rollout tail (rollout_tail_batched.hip): the same for B
// scenes of one layout, two launches of B workgroups
std::vector<int64_t> rollout_tail_batched_bounds() {
    return {rollout_tail_batched_max_scenes(),
            rollout_tail_batched_max_rows(),
            rollout_tail_batched_max_nodes()};
}

void rollout_tail_batched(
        int64_t kind, torch::Tensor states, torch::Tensor goal,
        torch::Tensor action, torch::Tensor explore,
        c10::optional<torch::Tensor> K, double dt, double r, double sl,
        double d2g, double act_lim, int64_t n_rec, double comm_radius,
        int64_t attr_kind, int64_t attr_dim, int64_t E_cap,
        std::vector<torch::Tensor> out, int64_t threads, int64_t topk) {
    TORCH_CHECK(kind >= 0 && kind <= 2,
                "rollout_tail_batched: unknown env kind ", kind);
    TORCH_CHECK(topk == -1 || (topk >= 1 && topk < (int64_t(1) << 31)),
                "rollout_tail_batched: topk must be -1 (no cap) or >= 1, "
                "got ", topk);
    const int64_t S = kind == 2 ? 6 : 4, P = kind == 2 ? 3 : 2;
    const int64_t A = kind == 2 ? 3 : 2, G = kind == 0 ? 2 : S;
    TORCH_CHECK(states.dim() == 3 && action.dim() == 3,
                "rollout_tail_batched: states (B, N, S) and action "
                "(B, n, A) expected");
    const int64_t B = states.size(0), N = states.size(1),
                  n = action.size(1);
    TORCH_CHECK(B >= 1 && B <= rollout_tail_batched_max_scenes(),
                "rollout_tail_batched: B must be in [1, ",
                rollout_tail_batched_max_scenes(), "], got ", B);
    CHECK_F32(states, B, N, S);
    CHECK_F32(goal, B, n, G);
    CHECK_F32(action, B, n, A);
    CHECK_IN(explore);
    TORCH_CHECK(explore.scalar_type() == torch::kInt32 &&
                explore.dim() == 1 && explore.size(0) == B,
                "rollout_tail_batched: explore must be int32 of shape (B,)");
    TORCH_CHECK(n >= 1 && n <= N && (kind != 0 || n == N),
                "rollout_tail_batched: bad agent count ", n, " for ", N,
                " nodes");
    const float* kptr = nullptr;
    if (kind != 1) {
        TORCH_CHECK(K.has_value(),
                    "rollout_tail_batched: this env needs the gain K");
        const torch::Tensor& Kt = K.value();
        CHECK_F32(Kt, A, S);
        kptr = Kt.data_ptr<float>();
    }
    TORCH_CHECK(n_rec >= 1 && n_rec <= n,
                "rollout_tail_batched: n_rec must be in [1, n]");
    TORCH_CHECK(n_rec <= rollout_tail_batched_max_rows() &&
                N <= rollout_tail_batched_max_nodes(),
                "rollout_tail_batched: scene (", n_rec, " receivers, ", N,
                " nodes) above the one-workgroup-per-scene bound (",
                rollout_tail_batched_max_rows(), ", ",
                rollout_tail_batched_max_nodes(), ")");
    TORCH_CHECK((attr_kind == 0 && attr_dim == S) ||
                (attr_kind == 1 && S == 4 && attr_dim == 5),
                "rollout_tail_batched: attr_kind/attr_dim mismatch");
    TORCH_CHECK(E_cap >= 0 && E_cap <= B * n_rec * (N - 1) + 64,
                "rollout_tail_batched: bad E_cap ", E_cap);
    TORCH_CHECK(threads == 256 || threads == 512 || threads == 1024,
                "rollout_tail_batched: threads must be 256, 512 or 1024");
    TORCH_CHECK(out.size() == 10, "out must be {new_states, u_ref_next, "
                "reward, reach, collision, edge_index, seg, edge_attr, "
                "flags, e_count}");
    const torch::Tensor &new_states = out[0], &u_ref_next = out[1],
        &reward = out[2], &reach = out[3], &collision = out[4],
        &edge_index = out[5], &seg = out[6], &edge_attr = out[7],
        &flags = out[8], &e_count = out[9];
    CHECK_F32(new_states, B, N, S);
    CHECK_F32(u_ref_next, B, n, A);
    CHECK_F32(reward, B, n);
    CHECK_BOOL(reach, B, n);
    CHECK_BOOL(collision, B, n);
    CHECK_F32(edge_attr, E_cap, attr_dim);
    CHECK_IN(edge_index); CHECK_IN(seg); CHECK_IN(flags); CHECK_IN(e_count);
    TORCH_CHECK(edge_index.scalar_type() == torch::kInt64 &&
                seg.scalar_type() == torch::kInt64 &&
                edge_index.sizes() == torch::IntArrayRef({2, E_cap}) &&
                seg.sizes() == torch::IntArrayRef({E_cap}),
                "rollout_tail_batched: edge_index (2, E_cap) / seg (E_cap,) "
                "int64 expected");
    TORCH_CHECK(flags.scalar_type() == torch::kInt32 &&
                flags.sizes() == torch::IntArrayRef({B, 3}),
                "rollout_tail_batched: flags must be int32 (B, 3)");
    TORCH_CHECK(e_count.scalar_type() == torch::kInt32 &&
                e_count.numel() == 1,
                "rollout_tail_batched: e_count must be int32 (1,)");
    const auto dev = states.device();
    for (const torch::Tensor& t : out)
        TORCH_CHECK(t.device() == dev,
                    "rollout_tail_batched: all tensors must be on one device");
    TORCH_CHECK(goal.device() == dev && action.device() == dev &&
                explore.device() == dev,
                "rollout_tail_batched: all tensors must be on one device");
    TORCH_CHECK(!K.has_value() || K->device() == dev,
                "rollout_tail_batched: all tensors must be on one device");
    TORCH_CHECK(new_states.data_ptr() != states.data_ptr(),
                "rollout_tail_batched: new_states must not alias states");
    // per-row counts: the hand-over between the two launches
    auto counts = torch::empty({B * n_rec},
                               states.options().dtype(torch::kInt32));
    // per-row cap thresholds, the same hand-over; only while the cap is live
    float* thr_ptr = nullptr;
    torch::Tensor thr;
    if (topk > 0 && topk < N) {
        thr = torch::empty({B * n_rec}, states.options());
        thr_ptr = thr.data_ptr<float>();
    }
    launch_rollout_tail_batched(
        (int)kind, states.data_ptr<float>(), goal.data_ptr<float>(),
        action.data_ptr<float>(), explore.data_ptr<int>(), kptr,
        new_states.data_ptr<float>(), u_ref_next.data_ptr<float>(),
        reward.data_ptr<float>(), reach.data_ptr<bool>(),
        collision.data_ptr<bool>(), counts.data_ptr<int>(), thr_ptr,
        edge_index.data_ptr<int64_t>(), seg.data_ptr<int64_t>(),
        edge_attr.data_ptr<float>(), flags.data_ptr<int>(),
        e_count.data_ptr<int>(), (int)B, (int)N, (int)n, (int)n_rec, (int)S,
        (int)G, (int)A, (int)P, (float)dt, (float)r, (float)sl, (float)d2g,
        (float)act_lim, (float)comm_radius, (int)attr_kind, (int)attr_dim,
        E_cap, (int)topk, (int)threads, current_stream());
}

// ---- MLP glue (mlp_glue.hip): padded bf16 GEMM inputs written directly
torch::Tensor edge_inputs_bf16(torch::Tensor x, torch::Tensor edge_index,
                               torch::Tensor edge_attr, int64_t rows_padded) {
    TORCH_CHECK(x.dim() == 2 && edge_attr.dim() == 2 &&
                edge_index.dim() == 2 && edge_index.size(0) == 2,
                "edge_inputs_bf16: x (N, nd), edge_index (2, E), edge_attr "
                "(E, ed) expected");
    const int64_t N = x.size(0), nd = x.size(1);
    const int64_t E = edge_index.size(1), ed = edge_attr.size(1);
    CHECK_F32(x, N, nd);
    CHECK_F32(edge_attr, E, ed);
    CHECK_IN(edge_index);
    TORCH_CHECK(edge_index.scalar_type() == torch::kInt64,
                "edge_index must be int64");
    TORCH_CHECK(rows_padded >= E, "rows_padded below the edge capacity");
    TORCH_CHECK(N < (int64_t(1) << 31) && nd < 65536 && ed < 65536,
                "edge_inputs_bf16: sizes out of range");
    auto out = torch::empty({rows_padded, 2 * nd + ed},
                            x.options().dtype(torch::kBFloat16));
    if (out.numel() > 0)
        launch_edge_inputs_bf16(x.data_ptr<float>(),
                                edge_index.data_ptr<int64_t>(),
                                edge_attr.data_ptr<float>(), out.data_ptr(),
                                (int)N, (int)nd, (int)ed, E, rows_padded,
                                current_stream());
    return out;
}

// out (rows_padded, D+nd) bf16 and the normalised attention weights att (E,)
// fp32.  Row r aggregates node idx[r] (int64, strictly increasing), or node
// r without an index.  att is written on the edges of those nodes only.
std::vector<torch::Tensor> attn_gamma_in_fwd(
        torch::Tensor msg, torch::Tensor gate, torch::Tensor seg,
        torch::Tensor x, c10::optional<torch::Tensor> idx, int64_t n_rows,
        int64_t num_nodes, int64_t rows_padded) {
    CHECK_IN(msg); CHECK_IN(gate); CHECK_IN(seg); CHECK_IN(x);
    TORCH_CHECK(msg.scalar_type() == torch::kBFloat16 && msg.dim() == 2,
                "msg must be bf16 (rows, D)");
    TORCH_CHECK(gate.scalar_type() == torch::kBFloat16 ||
                gate.scalar_type() == torch::kFloat32,
                "gate must be bf16 or fp32");
    TORCH_CHECK(seg.scalar_type() == torch::kInt64 && seg.dim() == 1,
                "seg must be int64 (E,)");
    TORCH_CHECK(x.scalar_type() == torch::kFloat32 && x.dim() == 2,
                "x must be fp32 (N, nd)");
    const int64_t E = seg.size(0), D = msg.size(1), nd = x.size(1);
    TORCH_CHECK(msg.size(0) >= E && gate.numel() >= E,
                "msg and gate must cover every edge slot");
    TORCH_CHECK(n_rows >= 0 && n_rows <= num_nodes &&
                num_nodes <= x.size(0) && n_rows <= rows_padded,
                "attn_aggregate_gamma_in: bad n_rows ", n_rows);
    const int64_t* iptr = nullptr;
    if (idx.has_value()) {
        CHECK_IN(idx.value());
        TORCH_CHECK(idx->scalar_type() == torch::kInt64 && idx->dim() == 1 &&
                    idx->size(0) == n_rows,
                    "idx must be int64 (n_rows,)");
        iptr = idx->data_ptr<int64_t>();
    }
    TORCH_CHECK(E < (int64_t(1) << 31) && rows_padded < (int64_t(1) << 31) &&
                num_nodes < (int64_t(1) << 31) &&
                E * D < (int64_t(1) << 40) && D + nd < (int64_t(1) << 24),
                "attn_aggregate_gamma_in: sizes out of range");
    auto out = torch::empty({rows_padded, D + nd}, msg.options());
    // per-edge softmax staging; only entries inside a segment are touched
    auto att = torch::empty({E}, x.options());
    if (rows_padded > 0)
        launch_attn_gamma_in(msg.data_ptr(), gate.data_ptr(),
                             gate.scalar_type() == torch::kBFloat16 ? 1 : 0,
                             seg.data_ptr<int64_t>(), x.data_ptr<float>(),
                             iptr, att.data_ptr<float>(), out.data_ptr(),
                             (int)E, (int)D, (int)nd, (int)n_rows,
                             (int)num_nodes, (int)rows_padded,
                             current_stream());
    return {out, att};
}

torch::Tensor attn_aggregate_gamma_in(torch::Tensor msg, torch::Tensor gate,
                                      torch::Tensor seg, torch::Tensor x,
                                      int64_t n_rows, int64_t num_nodes,
                                      int64_t rows_padded) {
    return attn_gamma_in_fwd(msg, gate, seg, x, c10::nullopt, n_rows,
                             num_nodes, rows_padded)[0];
}

// shared checks of the two backward launches; returns the idx pointer
static const int64_t* attn_bwd_checks(
        const torch::Tensor& dout, const torch::Tensor& att,
        const torch::Tensor& seg, const c10::optional<torch::Tensor>& idx,
        int64_t n_rows, int64_t num_nodes, int64_t D, int64_t rows) {
    CHECK_IN(dout); CHECK_IN(att); CHECK_IN(seg);
    TORCH_CHECK(dout.scalar_type() == torch::kBFloat16 && dout.dim() == 2 &&
                dout.size(1) >= D && dout.size(0) >= n_rows,
                "dout must be bf16 (>= n_rows, D + nd)");
    TORCH_CHECK(seg.scalar_type() == torch::kInt64 && seg.dim() == 1,
                "seg must be int64 (E,)");
    const int64_t E = seg.size(0);
    TORCH_CHECK(att.scalar_type() == torch::kFloat32 && att.numel() == E,
                "att must be fp32 (E,)");
    TORCH_CHECK(n_rows >= 1 && n_rows <= num_nodes && rows >= E,
                "attn_gamma_in_bwd: bad n_rows / rows");
    TORCH_CHECK(rows < (int64_t(1) << 31) && num_nodes < (int64_t(1) << 31) &&
                rows * D < (int64_t(1) << 40) &&
                dout.size(1) < (int64_t(1) << 24),
                "attn_gamma_in_bwd: sizes out of range");
    if (!idx.has_value()) return nullptr;
    CHECK_IN(idx.value());
    TORCH_CHECK(idx->scalar_type() == torch::kInt64 && idx->dim() == 1 &&
                idx->size(0) == n_rows, "idx must be int64 (n_rows,)");
    return idx->data_ptr<int64_t>();
}

// the caller's output buffer where one is given (tests prefill it), else a
// fresh one; every kernel that takes it writes every element
static torch::Tensor glue_out(const c10::optional<torch::Tensor>& out,
                              torch::IntArrayRef sizes,
                              const torch::TensorOptions& opts) {
    if (!out.has_value()) return torch::empty(sizes, opts);
    CHECK_IN(out.value());
    TORCH_CHECK(out->sizes() == sizes &&
                out->scalar_type() == opts.dtype().toScalarType(),
                "out has shape ", out->sizes(), ", expected ", sizes);
    return *out;
}

// dgate (rows, 1) bf16 for the gate MLP's output; rows = msg.size(0)
torch::Tensor attn_gamma_in_bwd_gate(
        torch::Tensor dout, torch::Tensor msg, torch::Tensor att,
        torch::Tensor seg, c10::optional<torch::Tensor> idx, int64_t n_rows,
        int64_t num_nodes, c10::optional<torch::Tensor> out = c10::nullopt) {
    CHECK_IN(msg);
    TORCH_CHECK(msg.scalar_type() == torch::kBFloat16 && msg.dim() == 2,
                "msg must be bf16 (rows, D)");
    const int64_t rows = msg.size(0), D = msg.size(1), E = seg.size(0);
    const int64_t* iptr = attn_bwd_checks(dout, att, seg, idx, n_rows,
                                          num_nodes, D, rows);
    auto dgate = glue_out(out, {rows, 1}, msg.options());
    auto stage = torch::empty({E}, att.options());
    launch_attn_gamma_in_bwd_gate(
        dout.data_ptr(), msg.data_ptr(), att.data_ptr<float>(),
        seg.data_ptr<int64_t>(), iptr, stage.data_ptr<float>(),
        dgate.data_ptr(), (int)E, (int)D, (int)(dout.size(1) - D),
        (int)n_rows, (int)num_nodes, (int)rows, current_stream());
    return dgate;
}

// dmsg (rows, D) bf16 for phi's output; dmsg_gate is the gate MLP's
// gradient for the same tensor.  round_prod: att * g is rounded to bf16
// before the two are added (a phi whose output was bf16)
torch::Tensor attn_gamma_in_bwd_msg(
        torch::Tensor dout, torch::Tensor att, torch::Tensor seg,
        c10::optional<torch::Tensor> idx, torch::Tensor dmsg_gate,
        int64_t n_rows, int64_t num_nodes, bool round_prod,
        c10::optional<torch::Tensor> out = c10::nullopt) {
    CHECK_IN(dmsg_gate);
    TORCH_CHECK(dmsg_gate.scalar_type() == torch::kBFloat16 &&
                dmsg_gate.dim() == 2, "dmsg_gate must be bf16 (rows, D)");
    const int64_t rows = dmsg_gate.size(0), D = dmsg_gate.size(1);
    const int64_t* iptr = attn_bwd_checks(dout, att, seg, idx, n_rows,
                                          num_nodes, D, rows);
    auto dmsg = glue_out(out, dmsg_gate.sizes(), dmsg_gate.options());
    TORCH_CHECK(dmsg.data_ptr() != dmsg_gate.data_ptr(),
                "out must not alias dmsg_gate");
    launch_attn_gamma_in_bwd_msg(
        dout.data_ptr(), att.data_ptr<float>(), seg.data_ptr<int64_t>(),
        iptr, dmsg_gate.data_ptr(), dmsg.data_ptr(), (int)seg.size(0),
        (int)D, (int)(dout.size(1) - D), (int)n_rows, (int)num_nodes,
        (int)rows, round_prod ? 1 : 0, current_stream());
    return dmsg;
}

torch::Tensor edge_inputs_bwd(torch::Tensor din, int64_t E, int64_t nd,
                              int64_t ed) {
    CHECK_IN(din);
    TORCH_CHECK(din.scalar_type() == torch::kBFloat16 && din.dim() == 2 &&
                nd >= 0 && ed >= 0 && din.size(1) == 2 * nd + ed &&
                E >= 0 && din.size(0) >= E,
                "edge_inputs_bwd: din must be bf16 (>= E, 2*nd+ed)");
    auto dea = torch::empty({E, ed}, din.options().dtype(torch::kFloat32));
    if (dea.numel() > 0)
        launch_edge_inputs_bwd(din.data_ptr(), dea.data_ptr<float>(), (int)nd,
                               (int)ed, E, current_stream());
    return dea;
}

torch::Tensor rows_cat_bwd(torch::Tensor din, int64_t Da, int64_t n_rows,
                           c10::optional<torch::Tensor> out = c10::nullopt) {
    CHECK_IN(din);
    TORCH_CHECK(din.scalar_type() == torch::kBFloat16 && din.dim() == 2 &&
                Da >= 0 && Da <= din.size(1) && n_rows >= 0 &&
                n_rows <= din.size(0),
                "rows_cat_bwd: din must be bf16 (rows, Da+Db)");
    auto da = glue_out(out, {din.size(0), Da}, din.options());
    if (da.numel() > 0)
        launch_rows_cat_bwd(din.data_ptr(), da.data_ptr(), (int)Da,
                            (int)(din.size(1) - Da), n_rows, din.size(0),
                            current_stream());
    return da;
}

// ---- MACBF actor glue (macbf_glue.hip): segment max of φ's padded bf16
// output straight into γ's padded bf16 input.  Row r is the max over the
// messages of node idx[r] (int64), or node r without an index; rows past
// n_rows and empty segments are zero.  Forward only.
torch::Tensor segmax_rows_bf16(torch::Tensor msg, torch::Tensor seg,
                               c10::optional<torch::Tensor> idx,
                               int64_t n_rows, int64_t num_nodes,
                               int64_t rows_padded) {
    CHECK_IN(msg); CHECK_IN(seg);
    TORCH_CHECK(!torch::GradMode::is_enabled() || !msg.requires_grad(),
                "segmax_rows_bf16 is forward only: call it without grad");
    TORCH_CHECK(msg.scalar_type() == torch::kBFloat16 && msg.dim() == 2,
                "msg must be bf16 (rows, D)");
    TORCH_CHECK(seg.scalar_type() == torch::kInt64 && seg.dim() == 1,
                "seg must be int64 (E,)");
    TORCH_CHECK(seg.device() == msg.device(),
                "segmax_rows_bf16: all tensors must be on one device");
    const int64_t E = seg.size(0), D = msg.size(1);
    TORCH_CHECK(msg.size(0) >= E, "msg must cover every edge slot");
    TORCH_CHECK(n_rows >= 0 && n_rows <= rows_padded && num_nodes >= 0,
                "segmax_rows_bf16: bad n_rows ", n_rows);
    const int64_t* iptr = nullptr;
    if (idx.has_value()) {
        CHECK_IN(idx.value());
        TORCH_CHECK(idx->scalar_type() == torch::kInt64 && idx->dim() == 1 &&
                    idx->size(0) == n_rows &&
                    idx->device() == msg.device(),
                    "idx must be int64 (n_rows,) on msg's device");
        iptr = idx->data_ptr<int64_t>();
    } else {
        TORCH_CHECK(n_rows <= num_nodes,
                    "segmax_rows_bf16: n_rows above num_nodes");
    }
    TORCH_CHECK(E < (int64_t(1) << 31) && rows_padded < (int64_t(1) << 31) &&
                num_nodes < (int64_t(1) << 31) && D < (int64_t(1) << 24) &&
                E * D < (int64_t(1) << 40),
                "segmax_rows_bf16: sizes out of range");
    auto out = torch::empty({rows_padded, D}, msg.options());
    if (out.numel() > 0)
        launch_segmax_rows_bf16(msg.data_ptr(), seg.data_ptr<int64_t>(), iptr,
                                out.data_ptr(), (int)E, (int)D, (int)n_rows,
                                (int)num_nodes, (int)rows_padded,
                                current_stream());
    return out;
}

torch::Tensor rows_cat_pad_bf16(torch::Tensor a, torch::Tensor b,
                                int64_t n_rows, int64_t rows_padded) {
    CHECK_IN(a); CHECK_IN(b);
    TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && a.dim() == 2,
                "a must be bf16 (rows, Da)");
    TORCH_CHECK(b.scalar_type() == torch::kFloat32 && b.dim() == 2,
                "b must be fp32 (rows, Db)");
    TORCH_CHECK(n_rows >= 0 && n_rows <= a.size(0) && n_rows <= b.size(0) &&
                n_rows <= rows_padded, "rows_cat_pad_bf16: bad n_rows ",
                n_rows);
    const int64_t Da = a.size(1), Db = b.size(1);
    TORCH_CHECK(Da + Db < (int64_t(1) << 24), "rows_cat_pad_bf16: too wide");
    auto out = torch::empty({rows_padded, Da + Db}, a.options());
    if (out.numel() > 0)
        launch_rows_cat_pad_bf16(a.data_ptr(), b.data_ptr<float>(),
                                 out.data_ptr(), (int)Da, (int)Db, n_rows,
                                 rows_padded, current_stream());
    return out;
}

// ---- one-launch bf16 mirror refresh (mlp_glue.hip)
// Host table for refresh_mirrors, one row per Linear; every tensor is
// checked here because the kernel sees only addresses.  ``biases`` entries
// may be None, then the layer's two bias mirrors are ignored.
torch::Tensor mirror_table(
        std::vector<torch::Tensor> weights,
        std::vector<torch::Tensor> mirrors,
        std::vector<c10::optional<torch::Tensor>> biases,
        std::vector<c10::optional<torch::Tensor>> bias_mirrors,
        std::vector<c10::optional<torch::Tensor>> bias_copies) {
    const size_t n = weights.size();
    TORCH_CHECK(mirrors.size() == n && biases.size() == n &&
                bias_mirrors.size() == n && bias_copies.size() == n,
                "mirror_table: list lengths differ");
    auto table = torch::zeros({(int64_t)n, 8}, torch::kInt64);
    auto* t = table.data_ptr<int64_t>();
    for (size_t i = 0; i < n; ++i, t += 8) {
        const torch::Tensor& w = weights[i];
        const torch::Tensor& wb = mirrors[i];
        CHECK_IN(w); CHECK_IN(wb);
        TORCH_CHECK(w.dim() == 2 && w.scalar_type() == torch::kFloat32,
                    "mirror_table: weight must be fp32 (rows, K)");
        const int64_t rows = w.size(0), K = w.size(1);
        const int64_t K64 = (K + 63) / 64 * 64;
        TORCH_CHECK(wb.scalar_type() == torch::kBFloat16 &&
                    wb.sizes() == torch::IntArrayRef({rows, K64}),
                    "mirror_table: mirror must be bf16 (rows, K64)");
        TORCH_CHECK(K64 < (int64_t(1) << 31), "mirror_table: K too large");
        t[0] = (int64_t)w.data_ptr();
        t[1] = (int64_t)wb.data_ptr();
        t[2] = rows; t[3] = K; t[4] = K64;
        if (biases[i].has_value()) {
            TORCH_CHECK(bias_mirrors[i].has_value() &&
                        bias_copies[i].has_value(),
                        "mirror_table: bias without mirrors");
            const torch::Tensor& b = *biases[i];
            const torch::Tensor& bb = *bias_mirrors[i];
            const torch::Tensor& b32 = *bias_copies[i];
            CHECK_F32(b, rows);
            CHECK_F32(b32, rows);
            CHECK_IN(bb);
            TORCH_CHECK(bb.scalar_type() == torch::kBFloat16 &&
                        bb.sizes() == torch::IntArrayRef({rows}),
                        "mirror_table: bias mirror must be bf16 (rows,)");
            TORCH_CHECK(b32.data_ptr() != b.data_ptr(),
                        "mirror_table: bias copy aliases the master");
            t[5] = (int64_t)b.data_ptr();
            t[6] = (int64_t)bb.data_ptr();
            t[7] = (int64_t)b32.data_ptr();
        }
    }
    return table;
}

void refresh_mirrors(torch::Tensor table, int64_t max_groups) {
    CHECK_IN(table);
    TORCH_CHECK(table.scalar_type() == torch::kInt64 && table.dim() == 2 &&
                table.size(1) == 8, "refresh_mirrors: table must be int64 "
                "(n, 8) as built by mirror_table");
    TORCH_CHECK(table.size(0) <= 65535, "refresh_mirrors: too many layers");
    if (table.size(0) == 0) return;
    launch_refresh_mirrors(
        reinterpret_cast<const long long*>(table.data_ptr<int64_t>()),
        (int)table.size(0), max_groups, current_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("fused_masks", &fused_masks,
          "batched safe/unsafe/collision agent masks in one pass");
    m.def("dubins_step", &dubins_step, "fused DubinsCar rollout step",
          py::arg("states"), py::arg("goal"), py::arg("action"),
          py::arg("dt"), py::arg("r"), py::arg("sl"), py::arg("d2g"),
          py::arg("act_lim"), py::arg("out") = py::none());
    m.def("car_step", &car_step, "fused SimpleCar rollout step",
          py::arg("states"), py::arg("goal"), py::arg("action"),
          py::arg("K"), py::arg("dt"), py::arg("r"), py::arg("sl"),
          py::arg("d2g"), py::arg("act_lim"), py::arg("out") = py::none());
    m.def("drone_step", &drone_step, "fused SimpleDrone rollout step",
          py::arg("states"), py::arg("goal"), py::arg("action"),
          py::arg("K"), py::arg("dt"), py::arg("r"), py::arg("sl"),
          py::arg("d2g"), py::arg("act_lim"), py::arg("out") = py::none());
    m.def("dubins_step_batched", &dubins_step_batched,
          "DubinsCar step of B scenes in one launch",
          py::arg("states"), py::arg("goal"), py::arg("action"),
          py::arg("active"), py::arg("dt"), py::arg("r"), py::arg("sl"),
          py::arg("d2g"), py::arg("act_lim"), py::arg("out") = py::none());
    m.def("car_step_batched", &car_step_batched,
          "SimpleCar step of B scenes in one launch",
          py::arg("states"), py::arg("goal"), py::arg("action"),
          py::arg("active"), py::arg("K"), py::arg("dt"), py::arg("r"),
          py::arg("sl"), py::arg("d2g"), py::arg("act_lim"),
          py::arg("out") = py::none());
    m.def("drone_step_batched", &drone_step_batched,
          "SimpleDrone step of B scenes in one launch",
          py::arg("states"), py::arg("goal"), py::arg("action"),
          py::arg("active"), py::arg("K"), py::arg("dt"), py::arg("r"),
          py::arg("sl"), py::arg("d2g"), py::arg("act_lim"),
          py::arg("out") = py::none());
    m.def("segment_attn_fwd", &segment_attn_fwd,
          "fused scatter-softmax + weighted scatter-sum (forward)");
    m.def("segment_attn_bwd", &segment_attn_bwd,
          "fused scatter-softmax + weighted scatter-sum (backward)");
    m.def("segment_max_fwd", &segment_max_fwd,
          "CSR segment max with argmax (forward)");
    m.def("segment_max_bwd", &segment_max_bwd,
          "CSR segment max scatter-back (backward)");
    m.def("build_graph", &build_graph,
          "batched dense radius graph + edge_attr (count/scan/fill)");
    m.def("build_graph_padded", &build_graph_padded,
          "capture-safe radius graph into fixed E_max buffers",
          py::arg("pos"), py::arg("states"), py::arg("B"), py::arg("n_rec"),
          py::arg("r"), py::arg("topk"), py::arg("attr_kind"),
          py::arg("attr_dim"), py::arg("E_max"),
          py::arg("out") = py::none());
    m.def("fused_linear", &fused_linear,
          "MFMA bf16 GEMM with fused bias + activation epilogue");
    m.def("reset_sample", &reset_sample,
          "greedy rejection sampling over a candidate pool (episode reset)",
          py::arg("cand"), py::arg("min_sep"), py::arg("avoid"),
          py::arg("avoid_dist"), py::arg("pts"), py::arg("count"));
    m.def("rollout_tail_batched", &rollout_tail_batched,
          "mask -> env step -> padded graph rebuild -> flags for B scenes, "
          "two launches of B workgroups",
          py::arg("kind"), py::arg("states"), py::arg("goal"),
          py::arg("action"), py::arg("explore"), py::arg("K"),
          py::arg("dt"), py::arg("r"), py::arg("sl"), py::arg("d2g"),
          py::arg("act_lim"), py::arg("n_rec"), py::arg("comm_radius"),
          py::arg("attr_kind"), py::arg("attr_dim"), py::arg("E_cap"),
          py::arg("out"), py::arg("threads") = 1024, py::arg("topk") = -1);
    m.def("rollout_tail_batched_bounds", &rollout_tail_batched_bounds,
          "(max scenes, max receiver rows, max nodes per scene)");
    m.def("rollout_tail", &rollout_tail,
          "mask -> env step -> padded graph rebuild -> flags, one launch",
          py::arg("kind"), py::arg("states"), py::arg("goal"),
          py::arg("action"), py::arg("K"), py::arg("dt"), py::arg("r"),
          py::arg("sl"), py::arg("d2g"), py::arg("act_lim"),
          py::arg("n_rec"), py::arg("comm_radius"), py::arg("attr_kind"),
          py::arg("attr_dim"), py::arg("E_max"), py::arg("out"),
          py::arg("threads") = 1024, py::arg("topk") = -1);
    m.def("rollout_tail_bounds", &rollout_tail_bounds,
          "(max receiver rows, max nodes) the single-workgroup tail takes");
    m.def("edge_inputs_bf16", &edge_inputs_bf16,
          "[x[dst], x[src], edge_attr] as zero-padded bf16 rows",
          py::arg("x"), py::arg("edge_index"), py::arg("edge_attr"),
          py::arg("rows_padded"));
    m.def("attn_aggregate_gamma_in", &attn_aggregate_gamma_in,
          "segment attention sum ++ x as zero-padded bf16 rows",
          py::arg("msg"), py::arg("gate"), py::arg("seg"), py::arg("x"),
          py::arg("n_rows"), py::arg("num_nodes"), py::arg("rows_padded"));
    m.def("attn_gamma_in_fwd", &attn_gamma_in_fwd,
          "attn_aggregate_gamma_in over optional row indices, keeping att",
          py::arg("msg"), py::arg("gate"), py::arg("seg"), py::arg("x"),
          py::arg("idx"), py::arg("n_rows"), py::arg("num_nodes"),
          py::arg("rows_padded"));
    m.def("attn_gamma_in_bwd_gate", &attn_gamma_in_bwd_gate,
          "gate gradient of attn_gamma_in_fwd as zero-padded bf16 rows",
          py::arg("dout"), py::arg("msg"), py::arg("att"), py::arg("seg"),
          py::arg("idx"), py::arg("n_rows"), py::arg("num_nodes"),
          py::arg("out") = py::none());
    m.def("attn_gamma_in_bwd_msg", &attn_gamma_in_bwd_msg,
          "message gradient of attn_gamma_in_fwd plus the gate MLP's",
          py::arg("dout"), py::arg("att"), py::arg("seg"), py::arg("idx"),
          py::arg("dmsg_gate"), py::arg("n_rows"), py::arg("num_nodes"),
          py::arg("round_prod"), py::arg("out") = py::none());
    m.def("edge_inputs_bwd", &edge_inputs_bwd,
          "edge_attr gradient of edge_inputs_bf16 (fp32)",
          py::arg("din"), py::arg("E"), py::arg("nd"), py::arg("ed"));
    m.def("rows_cat_bwd", &rows_cat_bwd,
          "gradient of rows_cat_pad_bf16's bf16 operand, zero pad rows",
          py::arg("din"), py::arg("Da"), py::arg("n_rows"),
          py::arg("out") = py::none());
    m.def("rows_cat_pad_bf16", &rows_cat_pad_bf16,
          "[a_bf16, b_fp32] as zero-padded bf16 rows",
          py::arg("a"), py::arg("b"), py::arg("n_rows"),
          py::arg("rows_padded"));
    m.def("segmax_rows_bf16", &segmax_rows_bf16,
          "segment max of bf16 messages as zero-padded bf16 rows (no grad)",
          py::arg("msg"), py::arg("seg"), py::arg("idx"), py::arg("n_rows"),
          py::arg("num_nodes"), py::arg("rows_padded"));
    m.def("mirror_table", &mirror_table,
          "checked host table (n, 8) int64 for refresh_mirrors");
    m.def("refresh_mirrors", &refresh_mirrors,
          "refresh every bf16 weight/bias mirror of a table in one launch",
          py::arg("table"), py::arg("max_groups"));
}
