// Python bindings of mipipe._C: the native runtime and the HIP kernels.
//
// Every kernel entry point validates shapes/dtypes/devices on the host before
// launching (a faulting kernel can take down every GPU on the node), allocates
// outputs through the torch caching allocator and launches on the current HIP
// stream of the tensors' device.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/HIPGeneratorImpl.h>
#include <ATen/core/Generator.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <mutex>
#include <optional>
#include <tuple>

#include "kernels/kernels.h"
#include "runtime/ipc.h"
#include "runtime/runtime.h"

namespace py = pybind11;
using at::Tensor;

namespace mipipe {
namespace {

#define MP_CHECK(cond, ...) TORCH_CHECK(cond, "mipipe: ", __VA_ARGS__)

hipStream_t cur_stream(const Tensor& t) { return at::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

// (seed, offset) from the torch device generator; `increment` philox words per
// thread are reserved so successive ops never reuse a counter.
std::pair<uint64_t, uint64_t> philox_draw(const at::Device& dev, uint64_t increment) {
  auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
      std::nullopt, at::cuda::detail::getDefaultCUDAGenerator(dev.index()));
  std::lock_guard<std::mutex> lock(gen->mutex_);
  return gen->philox_engine_inputs(increment);
}

void check_cuda(const Tensor& t, const char* name) {
  MP_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  MP_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_same(const Tensor& a, const Tensor& b, const char* an, const char* bn) {
  MP_CHECK(a.device() == b.device(), an, " and ", bn, " must be on the same device");
  MP_CHECK(a.scalar_type() == b.scalar_type(), an, " and ", bn, " must have the same dtype");
}

template <typename T>
T* ptr(const Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}
template <typename T>
const T* cptr(const Tensor& t) {
  return reinterpret_cast<const T*>(t.data_ptr());
}
template <typename T>
const T* optr(const std::optional<Tensor>& t) {
  return t.has_value() ? reinterpret_cast<const T*>(t->data_ptr()) : nullptr;
}

// ------------------------------------------------------------------ runtime
int64_t py_stream_acquire(int64_t device, int64_t priority) {
  return reinterpret_cast<int64_t>(rt::stream_acquire((int)device, (int)priority));
}

void py_stream_wait(int64_t waiting, int64_t waited, int64_t device) {
  rt::stream_wait(reinterpret_cast<hipStream_t>(waiting), reinterpret_cast<hipStream_t>(waited), (int)device);
}

void py_peer_copy(Tensor dst, Tensor src, int64_t src_stream, int64_t dst_stream, int64_t src_dev, int64_t dst_dev,
                  int64_t engine) {
  MP_CHECK(dst.is_contiguous() && src.is_contiguous(), "peer_copy needs contiguous tensors");
  MP_CHECK(dst.nbytes() == src.nbytes(), "peer_copy size mismatch");
  MP_CHECK(dst.is_cuda() && src.is_cuda(), "peer_copy needs device tensors");
  MP_CHECK(dst.get_device() == dst_dev && src.get_device() == src_dev, "peer_copy device mismatch");
  MP_CHECK(engine == rt::kCopySdma || engine == rt::kCopyBlit, "peer_copy: engine is 0 (sdma) or 1 (blit)");
  rt::peer_copy(dst.data_ptr(), (int)dst_dev, src.data_ptr(), (int)src_dev, src.nbytes(),
                reinterpret_cast<hipStream_t>(src_stream), reinterpret_cast<hipStream_t>(dst_stream), (int)engine);
}

void py_gpu_sleep(int64_t us) { mipipe::gpu_sleep(us, at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()); }

// ------------------------------------------------------------------ LayerNorm
std::tuple<Tensor, std::optional<Tensor>, Tensor, Tensor, int64_t, int64_t> py_layernorm_fwd(
    Tensor x, std::optional<Tensor> res, Tensor gamma, Tensor beta, double eps, double p, bool save_z) {
  check_cuda(x, "x");
  check_cuda(gamma, "gamma");
  check_cuda(beta, "beta");
  const int64_t cols = x.size(-1);
  const int64_t rows = x.numel() / cols;
  MP_CHECK(cols % 8 == 0, "layernorm: hidden size must be a multiple of 8, got ", cols);
  MP_CHECK(ln_max_vec((int)cols) > 0, "layernorm: hidden size too large: ", cols);
  MP_CHECK(gamma.numel() == cols && beta.numel() == cols, "layernorm: gamma/beta size mismatch");
  check_same(x, gamma, "x", "gamma");
  check_same(x, beta, "x", "beta");
  if (res.has_value()) {
    check_cuda(*res, "residual");
    check_same(x, *res, "x", "residual");
    MP_CHECK(res->numel() == x.numel(), "layernorm: residual shape mismatch");
  }
  MP_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1)");
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty_like(x);
  std::optional<Tensor> z;
  if (save_z) z = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({rows}, fopt);
  auto rstd = at::empty({rows}, fopt);
  uint64_t seed = 0, offset = 0;
  if (p > 0.0) std::tie(seed, offset) = philox_draw(x.device(), 4);
  auto s = cur_stream(x);
  if (rows == 0) return {y, z, mean, rstd, (int64_t)seed, (int64_t)offset};
  if (x.scalar_type() == at::kBFloat16) {
    LnArgs<bf16_t> a;
    a.x = cptr<bf16_t>(x); a.res = optr<bf16_t>(res); a.gamma = cptr<bf16_t>(gamma); a.beta = cptr<bf16_t>(beta);
    a.y = ptr<bf16_t>(y); a.z = z ? ptr<bf16_t>(*z) : nullptr; a.mean = ptr<float>(mean); a.rstd = ptr<float>(rstd);
    a.rows = (int)rows; a.cols = (int)cols; a.eps = (float)eps; a.p = (float)p; a.seed = seed; a.offset = offset;
    layernorm_fwd<bf16_t>(a, s);
  } else if (x.scalar_type() == at::kFloat) {
    LnArgs<float> a;
    a.x = cptr<float>(x); a.res = optr<float>(res); a.gamma = cptr<float>(gamma); a.beta = cptr<float>(beta);
    a.y = ptr<float>(y); a.z = z ? ptr<float>(*z) : nullptr; a.mean = ptr<float>(mean); a.rstd = ptr<float>(rstd);
    a.rows = (int)rows; a.cols = (int)cols; a.eps = (float)eps; a.p = (float)p; a.seed = seed; a.offset = offset;
    layernorm_fwd<float>(a, s);
  } else {
    MP_CHECK(false, "layernorm: unsupported dtype ", x.scalar_type());
  }
  return {y, z, mean, rstd, (int64_t)seed, (int64_t)offset};
}

// With acc_gamma/acc_beta (fp32 main_grad views) the parameter gradients are
// accumulated there and None is returned for them.
std::tuple<Tensor, std::optional<Tensor>, std::optional<Tensor>, std::optional<Tensor>> py_layernorm_bwd(
    Tensor dy, Tensor z, Tensor mean, Tensor rstd, Tensor gamma, double p, int64_t seed, int64_t offset,
    std::optional<Tensor> acc_gamma, std::optional<Tensor> acc_beta, std::optional<Tensor> addend) {
  check_cuda(dy, "dy");
  check_cuda(z, "z");
  check_same(dy, z, "dy", "z");
  check_same(dy, gamma, "dy", "gamma");
  const int64_t cols = dy.size(-1);
  const int64_t rows = dy.numel() / cols;
  MP_CHECK(z.numel() == dy.numel(), "layernorm_bwd: shape mismatch");
  MP_CHECK(mean.numel() == rows && rstd.numel() == rows, "layernorm_bwd: stats size mismatch");
  MP_CHECK(cols % 8 == 0 && ln_max_vec((int)cols) > 0, "layernorm_bwd: bad hidden size");
  if (addend) {
    check_same(dy, *addend, "dy", "addend");
    MP_CHECK(addend->numel() == dy.numel() && addend->is_contiguous(), "layernorm_bwd: addend must match dy");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
  auto dz = at::empty_like(dy);
  std::optional<Tensor> dx;
  if (p > 0.0) dx = at::empty_like(dy);
  const bool acc = acc_gamma.has_value();
  MP_CHECK(acc == acc_beta.has_value(), "layernorm_bwd: pass both accumulation targets or neither");
  if (acc) {
    for (auto* t : {&*acc_gamma, &*acc_beta}) {
      MP_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == at::kFloat && t->numel() == cols,
               "layernorm_bwd: accumulation targets must be contiguous fp32 [cols]");
    }
  }
  Tensor dgamma = acc ? *acc_gamma : at::empty_like(gamma);
  Tensor dbeta = acc ? *acc_beta : at::empty_like(gamma);
  const int nparts = std::max(1, ln_bwd_parts((int)rows, (int)cols));
  auto part = at::empty({2, nparts, cols}, dy.options().dtype(at::kFloat));
  auto s = cur_stream(dy);
  std::optional<Tensor> rg, rb;
  if (!acc) {
    rg = dgamma;
    rb = dbeta;
  }
  if (rows == 0) {
    if (!acc) {
      dgamma.zero_();
      dbeta.zero_();
    }
    return {dz, dx, rg, rb};
  }
  auto fill = [&](auto& a, auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    a.dy = cptr<T>(dy); a.z = cptr<T>(z); a.mean = cptr<float>(mean); a.rstd = cptr<float>(rstd);
    a.gamma = cptr<T>(gamma); a.dz = ptr<T>(dz); a.dx = dx ? ptr<T>(*dx) : nullptr;
    a.addend = addend ? cptr<T>(*addend) : nullptr;
    a.dgamma_part = ptr<float>(part); a.dbeta_part = ptr<float>(part) + (size_t)nparts * cols;
    a.dgamma = dgamma.data_ptr(); a.dbeta = dbeta.data_ptr();
    a.out_f32 = dgamma.scalar_type() == at::kFloat; a.accumulate = acc;
    a.rows = (int)rows; a.cols = (int)cols; a.nparts = nparts; a.p = (float)p;
    a.seed = (uint64_t)seed; a.offset = (uint64_t)offset;
  };
  if (dy.scalar_type() == at::kBFloat16) {
    LnBwdArgs<bf16_t> a;
    fill(a, (bf16_t*)nullptr);
    layernorm_bwd<bf16_t>(a, s);
  } else if (dy.scalar_type() == at::kFloat) {
    LnBwdArgs<float> a;
    fill(a, (float*)nullptr);
    layernorm_bwd<float>(a, s);
  } else {
    MP_CHECK(false, "layernorm_bwd: unsupported dtype");
  }
  return {dz, dx, rg, rb};
}

// ------------------------------------------------------------------ elementwise
template <typename F>
void dispatch_fb(const Tensor& t, const char* what, F&& f) {
  if (t.scalar_type() == at::kBFloat16) {
    f((bf16_t*)nullptr);
  } else if (t.scalar_type() == at::kFloat) {
    f((float*)nullptr);
  } else {
    MP_CHECK(false, what, ": unsupported dtype ", t.scalar_type());
  }
}

// ------------------------------------------------------------------ RMSNorm
std::tuple<Tensor, std::optional<Tensor>, Tensor, int64_t, int64_t> py_rmsnorm_fwd(
    Tensor x, std::optional<Tensor> res, Tensor gamma, double eps, double p, bool save_z) {
  check_cuda(x, "x");
  check_cuda(gamma, "gamma");
  MP_CHECK(x.dim() >= 1, "rmsnorm: x needs a hidden dimension");
  const int64_t cols = x.size(-1);
  MP_CHECK(cols > 0 && cols % 8 == 0, "rmsnorm: hidden size must be a positive multiple of 8, got ", cols);
  MP_CHECK(rms_max_vec((int)std::min<int64_t>(cols, 1 << 20)) > 0, "rmsnorm: hidden size too large: ", cols);
  const int64_t rows = x.numel() / cols;
  MP_CHECK(rows <= INT32_MAX, "rmsnorm: too many rows");
  MP_CHECK(gamma.numel() == cols, "rmsnorm: gamma size mismatch");
  check_same(x, gamma, "x", "gamma");
  if (res.has_value()) {
    check_cuda(*res, "residual");
    check_same(x, *res, "x", "residual");
    MP_CHECK(res->numel() == x.numel(), "rmsnorm: residual shape mismatch");
  }
  MP_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1)");
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty_like(x);
  std::optional<Tensor> z;
  if (save_z) z = at::empty_like(x);
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  uint64_t seed = 0, offset = 0;
  if (p > 0.0) std::tie(seed, offset) = philox_draw(x.device(), 4);
  auto s = cur_stream(x);
  if (rows == 0) return {y, z, rstd, (int64_t)seed, (int64_t)offset};
  dispatch_fb(x, "rmsnorm_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    RmsArgs<T> a;
    a.x = cptr<T>(x); a.res = optr<T>(res); a.gamma = cptr<T>(gamma);
    a.y = ptr<T>(y); a.z = z ? ptr<T>(*z) : nullptr; a.rstd = ptr<float>(rstd);
    a.rows = (int)rows; a.cols = (int)cols; a.eps = (float)eps; a.p = (float)p; a.seed = seed; a.offset = offset;
    rmsnorm_fwd<T>(a, s);
  });
  return {y, z, rstd, (int64_t)seed, (int64_t)offset};
}

// The sandwich norm y = res + RMSNorm(x) * gamma.  rstd (for rmsnorm_bwd on x) only with save.
std::tuple<Tensor, std::optional<Tensor>> py_rmsnorm_residual_fwd(Tensor x, Tensor res, Tensor gamma, double eps,
                                                                  bool save) {
  check_cuda(x, "x");
  check_cuda(res, "residual");
  check_cuda(gamma, "gamma");
  MP_CHECK(x.dim() >= 1, "rmsnorm_residual: x needs a hidden dimension");
  const int64_t cols = x.size(-1);
  MP_CHECK(cols > 0 && cols % 8 == 0, "rmsnorm_residual: hidden size must be a positive multiple of 8, got ", cols);
  MP_CHECK(rms_max_vec((int)std::min<int64_t>(cols, 1 << 20)) > 0, "rmsnorm_residual: hidden size too large: ", cols);
  const int64_t rows = x.numel() / cols;
  MP_CHECK(rows <= INT32_MAX, "rmsnorm_residual: too many rows");
  MP_CHECK(gamma.numel() == cols, "rmsnorm_residual: gamma size mismatch");
  check_same(x, gamma, "x", "gamma");
  check_same(x, res, "x", "residual");
  MP_CHECK(res.sizes() == x.sizes(), "rmsnorm_residual: residual shape mismatch");
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty_like(x);
  std::optional<Tensor> rstd;
  if (save) rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  if (rows == 0) return {y, rstd};
  auto s = cur_stream(x);
  dispatch_fb(x, "rmsnorm_residual_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    RmsArgs<T> a;
    a.x = cptr<T>(x); a.res = cptr<T>(res); a.gamma = cptr<T>(gamma);
    a.y = ptr<T>(y); a.rstd = rstd ? ptr<float>(*rstd) : nullptr;
    a.rows = (int)rows; a.cols = (int)cols; a.eps = (float)eps;
    rmsnorm_residual_fwd<T>(a, s);
  });
  return {y, rstd};
}

// With acc_gamma (a fp32 main_grad view) dgamma is accumulated there and None is returned for it.
std::tuple<Tensor, std::optional<Tensor>, std::optional<Tensor>> py_rmsnorm_bwd(
    Tensor dy, Tensor z, Tensor rstd, Tensor gamma, double p, int64_t seed, int64_t offset,
    std::optional<Tensor> acc_gamma, std::optional<Tensor> addend) {
  check_cuda(dy, "dy");
  check_cuda(z, "z");
  check_cuda(gamma, "gamma");
  check_cuda(rstd, "rstd");
  check_same(dy, z, "dy", "z");
  check_same(dy, gamma, "dy", "gamma");
  MP_CHECK(dy.dim() >= 1, "rmsnorm_bwd: dy needs a hidden dimension");
  const int64_t cols = dy.size(-1);
  MP_CHECK(cols > 0 && cols % 8 == 0 && rms_max_vec((int)std::min<int64_t>(cols, 1 << 20)) > 0,
           "rmsnorm_bwd: bad hidden size ", cols);
  const int64_t rows = dy.numel() / cols;
  MP_CHECK(rows <= INT32_MAX, "rmsnorm_bwd: too many rows");
  MP_CHECK(z.numel() == dy.numel(), "rmsnorm_bwd: shape mismatch");
  MP_CHECK(gamma.numel() == cols, "rmsnorm_bwd: gamma size mismatch");
  MP_CHECK(rstd.numel() == rows && rstd.scalar_type() == at::kFloat && rstd.device() == dy.device(),
           "rmsnorm_bwd: rstd must be fp32 [rows] on dy's device");
  MP_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1)");
  if (addend) {
    check_same(dy, *addend, "dy", "addend");
    MP_CHECK(addend->numel() == dy.numel() && addend->is_contiguous(), "rmsnorm_bwd: addend must match dy");
  }
  const bool acc = acc_gamma.has_value();
  if (acc) {
    MP_CHECK(acc_gamma->is_cuda() && acc_gamma->device() == dy.device() && acc_gamma->is_contiguous() &&
                 acc_gamma->scalar_type() == at::kFloat && acc_gamma->numel() == cols,
             "rmsnorm_bwd: the accumulation target must be contiguous fp32 [cols] on dy's device");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
  auto dz = at::empty_like(dy);
  std::optional<Tensor> dx;
  if (p > 0.0) dx = at::empty_like(dy);
  Tensor dgamma = acc ? *acc_gamma : at::empty_like(gamma);
  std::optional<Tensor> rg;
  if (!acc) rg = dgamma;
  if (rows == 0) {
    if (!acc) dgamma.zero_();
    return {dz, dx, rg};
  }
  const int nparts = std::max(1, rms_bwd_parts((int)rows, (int)cols));
  auto part = at::empty({nparts, cols}, dy.options().dtype(at::kFloat));
  auto s = cur_stream(dy);
  dispatch_fb(dy, "rmsnorm_bwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    RmsBwdArgs<T> a;
    a.dy = cptr<T>(dy); a.z = cptr<T>(z); a.rstd = cptr<float>(rstd); a.gamma = cptr<T>(gamma);
    a.dz = ptr<T>(dz); a.dx = dx ? ptr<T>(*dx) : nullptr; a.addend = addend ? cptr<T>(*addend) : nullptr;
    a.dgamma_part = ptr<float>(part); a.dgamma = dgamma.data_ptr();
    a.out_f32 = dgamma.scalar_type() == at::kFloat; a.accumulate = acc;
    a.rows = (int)rows; a.cols = (int)cols; a.nparts = nparts; a.p = (float)p;
    a.seed = (uint64_t)seed; a.offset = (uint64_t)offset;
    rmsnorm_bwd<T>(a, s);
  });
  return {dz, dx, rg};
}

// ------------------------------------------------------------------ SwiGLU / RoPE
Tensor py_swiglu_fwd(Tensor gu) {
  check_cuda(gu, "gu");
  MP_CHECK(gu.dim() >= 1, "swiglu: gu needs a feature dimension");
  const int64_t two_f = gu.size(-1);
  MP_CHECK(two_f > 0 && two_f % 16 == 0, "swiglu: the last dim is 2F with F a multiple of 8, got ", two_f);
  MP_CHECK(two_f / 2 <= INT32_MAX / 4, "swiglu: F too large");
  const int64_t F = two_f / 2, rows = gu.numel() / two_f;
  at::hip::HIPGuardMasqueradingAsCUDA guard(gu.device());
  auto shape = gu.sizes().vec();
  shape.back() = F;
  auto h = at::empty(shape, gu.options());
  auto s = cur_stream(gu);
  dispatch_fb(gu, "swiglu_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    swiglu_fwd<T>(cptr<T>(gu), ptr<T>(h), rows, (int)F, s);
  });
  return h;
}

Tensor py_swiglu_bwd(Tensor dh, Tensor gu) {
  check_cuda(dh, "dh");
  check_cuda(gu, "gu");
  check_same(dh, gu, "dh", "gu");
  MP_CHECK(gu.dim() >= 1 && dh.dim() >= 1, "swiglu_bwd: tensors need a feature dimension");
  const int64_t two_f = gu.size(-1);
  MP_CHECK(two_f > 0 && two_f % 16 == 0, "swiglu_bwd: the last dim of gu is 2F with F a multiple of 8, got ", two_f);
  MP_CHECK(two_f / 2 <= INT32_MAX / 4, "swiglu_bwd: F too large");
  const int64_t F = two_f / 2, rows = gu.numel() / two_f;
  MP_CHECK(dh.size(-1) == F && dh.numel() == rows * F, "swiglu_bwd: dh must be [rows, F]");
  at::hip::HIPGuardMasqueradingAsCUDA guard(gu.device());
  auto dgu = at::empty_like(gu);
  auto s = cur_stream(gu);
  dispatch_fb(gu, "swiglu_bwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    swiglu_bwd<T>(cptr<T>(dh), cptr<T>(gu), ptr<T>(dgu), rows, (int)F, s);
  });
  return dgu;
}

// GeGLU: the same checks, the tanh-GELU as the gate.
Tensor py_geglu_fwd(Tensor gu) {
  check_cuda(gu, "gu");
  MP_CHECK(gu.dim() >= 1, "geglu: gu needs a feature dimension");
  const int64_t two_f = gu.size(-1);
  MP_CHECK(two_f > 0 && two_f % 16 == 0, "geglu: the last dim is 2F with F a multiple of 8, got ", two_f);
  MP_CHECK(two_f / 2 <= INT32_MAX / 4, "geglu: F too large");
  const int64_t F = two_f / 2, rows = gu.numel() / two_f;
  at::hip::HIPGuardMasqueradingAsCUDA guard(gu.device());
  auto shape = gu.sizes().vec();
  shape.back() = F;
  auto h = at::empty(shape, gu.options());
  auto s = cur_stream(gu);
  dispatch_fb(gu, "geglu_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    geglu_fwd<T>(cptr<T>(gu), ptr<T>(h), rows, (int)F, s);
  });
  return h;
}

Tensor py_geglu_bwd(Tensor dh, Tensor gu) {
  check_cuda(dh, "dh");
  check_cuda(gu, "gu");
  check_same(dh, gu, "dh", "gu");
  MP_CHECK(gu.dim() >= 1 && dh.dim() >= 1, "geglu_bwd: tensors need a feature dimension");
  const int64_t two_f = gu.size(-1);
  MP_CHECK(two_f > 0 && two_f % 16 == 0, "geglu_bwd: the last dim of gu is 2F with F a multiple of 8, got ", two_f);
  MP_CHECK(two_f / 2 <= INT32_MAX / 4, "geglu_bwd: F too large");
  const int64_t F = two_f / 2, rows = gu.numel() / two_f;
  MP_CHECK(dh.size(-1) == F && dh.numel() == rows * F, "geglu_bwd: dh must be [rows, F]");
  at::hip::HIPGuardMasqueradingAsCUDA guard(gu.device());
  auto dgu = at::empty_like(gu);
  auto s = cur_stream(gu);
  dispatch_fb(gu, "geglu_bwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    geglu_bwd<T>(cptr<T>(dh), cptr<T>(gu), ptr<T>(dgu), rows, (int)F, s);
  });
  return dgu;
}

// x [B, S, heads, D] with the first n_rot heads of a token rotated and the rest passed through.
// out: None (a fresh tensor, the rest copied) or a tensor of x's layout; out being x itself rotates in place.
Tensor rope_impl(Tensor x, Tensor cos, Tensor sin, std::optional<Tensor> out, int64_t n_rot, int64_t pos0, bool inverse,
                 const char* name) {
  check_cuda(x, "qkv");
  check_cuda(cos, "cos");
  check_cuda(sin, "sin");
  const int64_t B = x.size(0), S = x.size(1), heads = x.size(2), D = x.size(3);
  MP_CHECK(n_rot >= 0 && n_rot <= heads, name, ": n_rot must be in [0, heads], got ", n_rot);
  MP_CHECK(D > 0 && D % 16 == 0, name, ": head dim must be a multiple of 16, got ", D);
  MP_CHECK(S <= INT32_MAX / 2 && heads * D <= INT32_MAX / 8 * 3, name, ": shape too large");
  MP_CHECK(pos0 >= 0 && pos0 <= INT32_MAX / 2, name, ": bad pos0 ", pos0);
  for (auto* t : {&cos, &sin}) {
    MP_CHECK(t->scalar_type() == at::kFloat && t->dim() == 2 && t->size(1) == D / 2 && t->size(0) >= pos0 + S &&
                 t->device() == x.device(),
             name, ": cos / sin must be fp32 [>= pos0 + S, D / 2] on qkv's device");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor o;
  if (out.has_value()) {
    o = *out;
    check_cuda(o, "out");
    check_same(x, o, "qkv", "out");
    MP_CHECK(o.sizes() == x.sizes(), name, ": out must have qkv's shape");
    // the same tensor or a disjoint one: a partial overlap would race
    if (o.data_ptr() != x.data_ptr()) {
      const char* a = static_cast<const char*>(x.data_ptr());
      const char* b = static_cast<const char*>(o.data_ptr());
      const int64_t n = (int64_t)x.nbytes();
      MP_CHECK(b + n <= a || a + n <= b, name, ": out partly overlaps qkv");
    }
  } else {
    o = at::empty_like(x);
  }
  auto s = cur_stream(x);
  dispatch_fb(x, name, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    rope_heads<T>(cptr<T>(x), cptr<float>(cos), cptr<float>(sin), ptr<T>(o), B, (int)S, (int)n_rot,
                  (int)(heads - n_rot), (int)D, (int)pos0, inverse, s);
  });
  return o;
}

// qkv [B, S, 3, H, D]: Q and K rotated, V passed through.
Tensor py_rope_packed(Tensor qkv, Tensor cos, Tensor sin, std::optional<Tensor> out, int64_t pos0, bool inverse) {
  MP_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "rope_packed: qkv must be [B, S, 3, H, D]");
  const int64_t H = qkv.size(3);
  const std::vector<int64_t> shape4 = {qkv.size(0), qkv.size(1), 3 * H, qkv.size(4)};
  MP_CHECK(qkv.is_contiguous(), "rope_packed: qkv must be contiguous");
  std::optional<Tensor> out4;
  if (out.has_value()) {
    MP_CHECK(out->sizes() == qkv.sizes() && out->is_contiguous(), "rope_packed: out must have qkv's shape and layout");
    out4 = out->view(shape4);
  }
  Tensor o = rope_impl(qkv.view(shape4), cos, sin, out4, 2 * H, pos0, inverse, "rope_packed");
  return out.has_value() ? *out : o.view(qkv.sizes());
}

// x [B, S, heads, D] (the grouped-query projection [B, S, H + 2 Hkv, D] with n_rot = H + Hkv).
Tensor py_rope_heads(Tensor x, Tensor cos, Tensor sin, std::optional<Tensor> out, int64_t n_rot, int64_t pos0,
                     bool inverse) {
  MP_CHECK(x.dim() == 4 && x.is_contiguous() && (!out.has_value() || out->is_contiguous()),
           "rope_heads: x (and out) must be contiguous [B, S, heads, D]");
  return rope_impl(x, cos, sin, out, n_rot, pos0, inverse, "rope_heads");
}

// ------------------------------------------------------------------ QK-norm
// The checks the forward and the backward share: x [B, S, heads, D] contiguous with the first n_q heads Q and the
// next n_k heads K, both weights [D] of x's dtype, tables (both or neither) fp32 [>= pos0 + S, D / 2].
void qknorm_check(const Tensor& x, const Tensor& wq, const Tensor& wk, const std::optional<Tensor>& cos,
                  const std::optional<Tensor>& sin, int64_t n_q, int64_t n_k, int64_t pos0, const char* name) {
  check_cuda(x, "x");
  check_cuda(wq, "wq");
  check_cuda(wk, "wk");
  check_same(x, wq, "x", "wq");
  check_same(x, wk, "x", "wk");
  MP_CHECK(x.dim() == 4, name, ": x must be [B, S, heads, D]");
  const int64_t S = x.size(1), heads = x.size(2), D = x.size(3);
  MP_CHECK(n_q >= 0 && n_k >= 0 && n_q + n_k <= heads, name, ": n_q + n_k must be in [0, heads], got ", n_q, " + ", n_k,
           " of ", heads);
  MP_CHECK(qknorm_supported((int)std::min<int64_t>(D, 1 << 20)), name, ": head dim must be 16, 32, 64, 128 or 256, got ", D);
  MP_CHECK(wq.numel() == D && wk.numel() == D, name, ": wq and wk must hold D = ", D, " values");
  MP_CHECK(S <= INT32_MAX / 2 && heads * D <= INT32_MAX / 8 * 3 && x.numel() / D <= (int64_t)1 << 40, name,
           ": shape too large");
  MP_CHECK(pos0 >= 0 && pos0 <= INT32_MAX / 2, name, ": bad pos0 ", pos0);
  MP_CHECK(cos.has_value() == sin.has_value(), name, ": give both cos and sin, or neither");
  for (auto* t : {&cos, &sin}) {
    if (!t->has_value()) continue;
    const Tensor& v = **t;
    MP_CHECK(v.is_cuda() && v.is_contiguous() && v.scalar_type() == at::kFloat && v.dim() == 2 && v.size(1) == D / 2 &&
                 v.size(0) >= pos0 + S && v.device() == x.device(),
             name, ": cos / sin must be contiguous fp32 [>= pos0 + S, D / 2] on x's device");
    MP_CHECK(reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0, name, ": cos / sin must be 16-byte aligned");
  }
  for (auto* t : {&x, &wq, &wk})
    MP_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, name, ": x, wq and wk must be 16-byte aligned");
}

// (y, rstd): out None (a fresh tensor, V copied) or x itself / a disjoint tensor of x's layout; rstd fp32
// [B * S, n_q + n_k] only with save_rstd (a forward under no_grad allocates none).
std::tuple<Tensor, std::optional<Tensor>> py_qk_norm_rope_fwd(Tensor x, Tensor wq, Tensor wk, double eps,
                                                              std::optional<Tensor> cos, std::optional<Tensor> sin,
                                                              std::optional<Tensor> out, int64_t n_q, int64_t n_k,
                                                              int64_t pos0, bool save_rstd) {
  const char* name = "qk_norm_rope_fwd";
  qknorm_check(x, wq, wk, cos, sin, n_q, n_k, pos0, name);
  const int64_t B = x.size(0), S = x.size(1), heads = x.size(2), D = x.size(3);
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor o;
  if (out.has_value()) {
    o = *out;
    check_cuda(o, "out");
    check_same(x, o, "x", "out");
    MP_CHECK(o.sizes() == x.sizes(), name, ": out must have x's shape");
    if (o.data_ptr() != x.data_ptr()) {  // the same tensor or a disjoint one: a partial overlap would race
      const char* a = static_cast<const char*>(x.data_ptr());
      const char* b = static_cast<const char*>(o.data_ptr());
      const int64_t n = (int64_t)x.nbytes();
      MP_CHECK(b + n <= a || a + n <= b, name, ": out partly overlaps x");
      MP_CHECK(reinterpret_cast<uintptr_t>(o.data_ptr()) % 16 == 0, name, ": out must be 16-byte aligned");
    }
  } else {
    o = at::empty_like(x);
  }
  std::optional<Tensor> rstd;
  if (save_rstd) rstd = at::empty({B * S, n_q + n_k}, x.options().dtype(at::kFloat));
  auto s = cur_stream(x);
  dispatch_fb(x, name, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    qknorm_rope_fwd<T>(cptr<T>(x), cptr<T>(wq), cptr<T>(wk), optr<float>(cos), optr<float>(sin), ptr<T>(o),
                       rstd ? ptr<float>(*rstd) : nullptr, B * S, (int)S, (int)n_q, (int)n_k, (int)(heads - n_q - n_k),
                       (int)D, (int)pos0, (float)eps, s);
  });
  return {o, rstd};
}

// (dx, dwq, dwk).  With acc_q / acc_k (fp32 main_grad views [D]) that weight's gradient is accumulated there and
// None is returned for it; otherwise it comes back in the weights' dtype.
std::tuple<Tensor, std::optional<Tensor>, std::optional<Tensor>> py_qk_norm_rope_bwd(
    Tensor dout, Tensor x, Tensor rstd, Tensor wq, Tensor wk, std::optional<Tensor> cos, std::optional<Tensor> sin,
    int64_t n_q, int64_t n_k, int64_t pos0, std::optional<Tensor> acc_q, std::optional<Tensor> acc_k) {
  const char* name = "qk_norm_rope_bwd";
  qknorm_check(x, wq, wk, cos, sin, n_q, n_k, pos0, name);
  check_cuda(dout, "dout");
  check_cuda(rstd, "rstd");
  check_same(x, dout, "x", "dout");
  MP_CHECK(dout.sizes() == x.sizes(), name, ": dout must have x's shape");
  MP_CHECK(reinterpret_cast<uintptr_t>(dout.data_ptr()) % 16 == 0, name, ": dout must be 16-byte aligned");
  const int64_t B = x.size(0), S = x.size(1), heads = x.size(2), D = x.size(3);
  MP_CHECK(rstd.scalar_type() == at::kFloat && rstd.numel() == B * S * (n_q + n_k) && rstd.device() == x.device(),
           name, ": rstd must be fp32 [B * S, n_q + n_k] on x's device");
  for (auto* a : {&acc_q, &acc_k}) {
    if (!a->has_value()) continue;
    const Tensor& v = **a;
    MP_CHECK(v.is_cuda() && v.device() == x.device() && v.is_contiguous() && v.scalar_type() == at::kFloat &&
                 v.numel() == D,
             name, ": an accumulation target must be contiguous fp32 [D] on x's device");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto dx = at::empty_like(x);
  Tensor dwq = acc_q ? *acc_q : at::empty_like(wq);
  Tensor dwk = acc_k ? *acc_k : at::empty_like(wk);
  std::optional<Tensor> rq, rk;
  if (!acc_q) rq = dwq;
  if (!acc_k) rk = dwk;
  if (x.numel() == 0) {
    if (!acc_q) dwq.zero_();
    if (!acc_k) dwk.zero_();
    return {dx, rq, rk};
  }
  const int n_v = (int)(heads - n_q - n_k);
  const int nparts = qknorm_bwd_parts(B * S, (int)n_q, (int)n_k, n_v, (int)D);
  auto part = at::empty({2, nparts, D}, x.options().dtype(at::kFloat));
  float* part_q = ptr<float>(part);
  float* part_k = part_q + (int64_t)nparts * D;
  auto s = cur_stream(x);
  dispatch_fb(x, name, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    qknorm_rope_bwd<T>(cptr<T>(dout), cptr<T>(x), cptr<float>(rstd), cptr<T>(wq), cptr<T>(wk), optr<float>(cos),
                       optr<float>(sin), ptr<T>(dx), part_q, part_k, nparts, B * S, (int)S, (int)n_q, (int)n_k, n_v,
                       (int)D, (int)pos0, s);
  });
  const bool f32_q = dwq.scalar_type() == at::kFloat, f32_k = dwk.scalar_type() == at::kFloat;
  if (f32_q == f32_k && acc_q.has_value() == acc_k.has_value()) {
    reduce_parts(part_q, part_k, nparts, (int)D, dwq.data_ptr(), dwk.data_ptr(), f32_q, acc_q.has_value(), s);
  } else {  // one weight accumulates into its fp32 main_grad, the other is stored: one pass each
    reduce_parts(part_q, nullptr, nparts, (int)D, dwq.data_ptr(), nullptr, f32_q, acc_q.has_value(), s);
    reduce_parts(part_k, nullptr, nparts, (int)D, dwk.data_ptr(), nullptr, f32_k, acc_k.has_value(), s);
  }
  return {dx, rq, rk};
}

// ------------------------------------------------------------------ mixture of experts
void moe_check_i32(const Tensor& t, const Tensor& like, int64_t numel, const char* name, const char* what) {
  check_cuda(t, what);
  MP_CHECK(t.scalar_type() == at::kInt && t.device() == like.device() && t.numel() == numel, name, ": ", what,
           " must be int32 with ", numel, " entries on the same device");
}
void moe_check_f32(const Tensor& t, const Tensor& like, int64_t numel, const char* name, const char* what) {
  check_cuda(t, what);
  MP_CHECK(t.scalar_type() == at::kFloat && t.device() == like.device() && t.numel() == numel, name, ": ", what,
           " must be fp32 with ", numel, " entries on the same device");
}
void moe_check_rows(const Tensor& t, const char* name, const char* what) {
  check_cuda(t, what);
  MP_CHECK(t.dim() == 2, name, ": ", what, " must be 2-D");
  MP_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat, name, ": unsupported dtype ",
           t.scalar_type());
  const int64_t E = t.size(1);
  MP_CHECK(E > 0 && E <= (1 << 24) && (E * t.element_size()) % 16 == 0, name, ": the width of ", what,
           " must fill whole 16-byte vectors (a multiple of 8; fp32: of 4), got ", E);
  MP_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, ": ", what, " must be 16-byte aligned");
}

// (idx int32 [T, k], gate fp32 [T, k], probs_sum fp32 [Ne]) of logits [T, Ne].
std::tuple<Tensor, Tensor, Tensor> py_moe_route_fwd(Tensor logits, int64_t k) {
  const char* name = "moe_route_fwd";
  check_cuda(logits, "logits");
  MP_CHECK(logits.dim() == 2, name, ": logits must be [T, Ne]");
  const int64_t T = logits.size(0), Ne = logits.size(1);
  MP_CHECK(Ne <= 256 && k <= 8 && moe_route_supported((int)Ne, (int)k), name,
           ": needs 2 <= Ne <= 256 and 1 <= k <= min(8, Ne), got Ne=", Ne, ", k=", k);
  MP_CHECK(T * Ne < (int64_t(1) << 40), name, ": too many tokens");
  at::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  auto idx = at::empty({T, k}, logits.options().dtype(at::kInt));
  auto gate = at::empty({T, k}, logits.options().dtype(at::kFloat));
  auto probs = at::empty({Ne}, logits.options().dtype(at::kFloat));
  if (T == 0) {
    probs.zero_();
    return {idx, gate, probs};
  }
  const int nparts = moe_route_parts(T, (int)Ne);
  auto part = at::empty({nparts, Ne}, logits.options().dtype(at::kFloat));
  auto s = cur_stream(logits);
  dispatch_fb(logits, name, [&](auto* tag) {
    using T_ = std::remove_pointer_t<decltype(tag)>;
    moe_route_fwd<T_>(cptr<T_>(logits), ptr<int32_t>(idx), ptr<float>(gate), ptr<float>(part), nparts, T, (int)Ne,
                      (int)k, s);
  });
  reduce_parts(ptr<float>(part), nullptr, nparts, (int)Ne, probs.data_ptr(), nullptr, true, false, s);
  return {idx, gate, probs};
}

Tensor py_moe_route_bwd(Tensor logits, Tensor idx, Tensor gate, Tensor dgate, std::optional<Tensor> dprobs) {
  const char* name = "moe_route_bwd";
  check_cuda(logits, "logits");
  MP_CHECK(logits.dim() == 2 && idx.dim() == 2 && idx.size(0) == logits.size(0), name,
           ": logits must be [T, Ne] and idx [T, k]");
  const int64_t T = logits.size(0), Ne = logits.size(1), k = idx.size(1);
  MP_CHECK(Ne <= 256 && k <= 8 && moe_route_supported((int)Ne, (int)k), name,
           ": needs 2 <= Ne <= 256 and 1 <= k <= min(8, Ne), got Ne=", Ne, ", k=", k);
  moe_check_i32(idx, logits, T * k, name, "idx");
  moe_check_f32(gate, logits, T * k, name, "gate");
  moe_check_f32(dgate, logits, T * k, name, "dgate");
  if (dprobs.has_value()) moe_check_f32(*dprobs, logits, Ne, name, "dprobs");
  at::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  auto dlogits = at::empty_like(logits);
  auto s = cur_stream(logits);
  dispatch_fb(logits, name, [&](auto* tag) {
    using T_ = std::remove_pointer_t<decltype(tag)>;
    moe_route_bwd<T_>(cptr<T_>(logits), cptr<int32_t>(idx), cptr<float>(gate), cptr<float>(dgate),
                      optr<float>(dprobs), ptr<T_>(dlogits), T, (int)Ne, (int)k, s);
  });
  return dlogits;
}

// (slot int32 [T, k], src int32 [Ne * C], counts int32 [Ne]) of idx [T, k].
std::tuple<Tensor, Tensor, Tensor> py_moe_assign(Tensor idx, int64_t n_experts, int64_t capacity) {
  const char* name = "moe_assign";
  check_cuda(idx, "idx");
  MP_CHECK(idx.dim() == 2 && idx.scalar_type() == at::kInt, name, ": idx must be int32 [T, k]");
  const int64_t T = idx.size(0), k = idx.size(1);
  MP_CHECK(n_experts <= 256 && k <= 8 && moe_route_supported((int)n_experts, (int)k), name,
           ": needs 2 <= Ne <= 256 and 1 <= k <= min(8, Ne), got Ne=", n_experts, ", k=", k);
  MP_CHECK(capacity >= 1 && n_experts * capacity < (int64_t(1) << 31), name,
           ": needs capacity >= 1 and Ne * capacity < 2^31, got ", capacity);
  MP_CHECK(T * k < (int64_t(1) << 31), name, ": T * k must be below 2^31");
  at::hip::HIPGuardMasqueradingAsCUDA guard(idx.device());
  auto slot = at::empty({T, k}, idx.options());
  auto src = at::empty({n_experts * capacity}, idx.options());
  auto counts = at::empty({n_experts}, idx.options());
  auto ws = at::empty({(int64_t)moe_assign_blocks(T, (int)k), n_experts}, idx.options());
  moe_assign(cptr<int32_t>(idx), ptr<int32_t>(slot), ptr<int32_t>(src), ptr<int32_t>(counts), ptr<int32_t>(ws), T,
             (int)k, (int)n_experts, (int)capacity, cur_stream(idx));
  return {slot, src, counts};
}

// The sorted layout (kernels.h): (slot [T, k], src [rows], counts [Ne], offsets [Ne + 1], tile_expert [rows / 128]).
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> py_moe_assign_sorted(Tensor idx, int64_t n_experts, int64_t rows) {
  const char* name = "moe_assign_sorted";
  check_cuda(idx, "idx");
  MP_CHECK(idx.dim() == 2 && idx.scalar_type() == at::kInt, name, ": idx must be int32 [T, k]");
  const int64_t T = idx.size(0), k = idx.size(1);
  MP_CHECK(n_experts <= 256 && k <= 8 && moe_route_supported((int)n_experts, (int)k), name,
           ": needs 2 <= Ne <= 256 and 1 <= k <= min(8, Ne), got Ne=", n_experts, ", k=", k);
  MP_CHECK(T * k < (int64_t(1) << 31), name, ": T * k must be below 2^31");
  // every count vector fits: sum_e ceil128(c_e) <= 128 * (n + (T k - n) / 128), n = min(Ne, T k)
  const int64_t n = std::min<int64_t>(n_experts, T * k);
  MP_CHECK(rows % 128 == 0 && rows >= 128 * (n + (T * k - n) / 128) && rows < (int64_t(1) << 31), name,
           ": rows must be a multiple of 128, at least 128 * (n + (T k - n) / 128) and below 2^31, got ", rows);
  at::hip::HIPGuardMasqueradingAsCUDA guard(idx.device());
  auto slot = at::empty({T, k}, idx.options());
  auto src = at::empty({rows}, idx.options());
  auto counts = at::empty({n_experts}, idx.options());
  auto offsets = at::empty({n_experts + 1}, idx.options());
  auto tile_expert = at::empty({rows / 128}, idx.options());
  auto ws = at::empty({(int64_t)moe_assign_blocks(T, (int)k), n_experts}, idx.options());
  moe_assign_sorted(cptr<int32_t>(idx), ptr<int32_t>(slot), ptr<int32_t>(src), ptr<int32_t>(counts),
                    ptr<int32_t>(offsets), ptr<int32_t>(tile_expert), ptr<int32_t>(ws), T, (int)k, (int)n_experts,
                    (int)rows, cur_stream(idx));
  return {slot, src, counts, offsets, tile_expert};
}

// ------------------------------------------------------------------ grouped GEMM
void grouped_check_table(const Tensor& t, const Tensor& like, int64_t n, at::ScalarType st, const char* name,
                         const char* what) {
  MP_CHECK(t.is_cuda() && t.is_contiguous() && t.device() == like.device() && t.scalar_type() == st &&
               t.dim() == 1 && t.numel() == n,
           name, ": ", what, " must be a contiguous ", st, " [", n, "] tensor on the operands' device");
}

void grouped_check_rows(const Tensor& t, const char* name, const char* what) {
  check_cuda(t, what);
  MP_CHECK(t.dim() == 2 && t.scalar_type() == at::kBFloat16, name, ": ", what, " must be bf16 [rows, width]");
  MP_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, ": ", what, " must be 16-byte aligned");
}

// y [R, n_out] = a [R, Kred] . op(W_e) per 128-row tile, e = tile_expert[tile] (zeros for -1).  wptrs [Ne]: the
// experts' weight pointers, each a contiguous bf16 [n_out, Kred] (w_kc, the forward) or [Kred, n_out] (the dgrad).
// The caller keeps the weights alive and answers for the table.
Tensor py_grouped_gemm_rows(Tensor a, Tensor wptrs, Tensor tile_expert, int64_t n_out, bool w_kc) {
  const char* name = "grouped_gemm_rows";
  grouped_check_rows(a, name, "a");
  const int64_t R = a.size(0), Kred = a.size(1), Ne = wptrs.numel();
  MP_CHECK(grouped_gemm_supported(R, n_out, Kred), name, ": needs rows % 128 == 0, n_out % 128 == 0 and a reduction "
           "width % 64 == 0, got rows=", R, ", n_out=", n_out, ", reduction=", Kred);
  MP_CHECK(Ne >= 1 && Ne < (1 << 16), name, ": needs 1 <= Ne < 65536 experts, got ", Ne);
  grouped_check_table(wptrs, a, Ne, at::kLong, name, "wptrs");
  grouped_check_table(tile_expert, a, R / 128, at::kInt, name, "tile_expert");
  at::hip::HIPGuardMasqueradingAsCUDA guard(a.device());
  auto y = at::empty({R, n_out}, a.options());
  grouped_gemm_rows(cptr<bf16_t>(a), cptr<int64_t>(wptrs), cptr<int32_t>(tile_expert), ptr<bf16_t>(y), R, n_out, Kred,
                    (int)Ne, w_kc, cur_stream(a));
  return y;
}

// dW_e [N, K] fp32 = or += dy[rows_e]^T x[rows_e], rows_e = [offsets[e], offsets[e + 1]).  With `optrs` (int64 [Ne])
// the experts' outputs are those pointers (fp32 [N, K] each, 16-byte aligned; the caller answers for them) and
// nothing is returned; without it a fresh fp32 [Ne, N, K] is written (store mode only) and returned.
std::optional<Tensor> py_grouped_gemm_wgrad(Tensor dy, Tensor x, Tensor offsets, std::optional<Tensor> optrs,
                                            bool accumulate) {
  const char* name = "grouped_gemm_wgrad";
  grouped_check_rows(dy, name, "dy");
  grouped_check_rows(x, name, "x");
  MP_CHECK(dy.device() == x.device(), name, ": dy and x must be on the same device");
  const int64_t R = dy.size(0), N = dy.size(1), K = x.size(1), Ne = offsets.numel() - 1;
  MP_CHECK(x.size(0) == R, name, ": dy has ", R, " rows, x ", x.size(0));
  MP_CHECK(R > 0 && R % 128 == 0 && N > 0 && N % 128 == 0 && K > 0 && K % 128 == 0 && R < (int64_t(1) << 31) &&
               (N / 128) * (K / 128) < (int64_t(1) << 31),
           name, ": needs rows, N and K to be multiples of 128, got ", R, ", ", N, ", ", K);
  MP_CHECK(Ne >= 1 && Ne < (1 << 16), name, ": needs 1 <= Ne < 65536 experts, got ", Ne);
  grouped_check_table(offsets, dy, Ne + 1, at::kInt, name, "offsets");
  MP_CHECK(optrs.has_value() || !accumulate, name, ": accumulate needs the table of outputs");
  at::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
  std::optional<Tensor> out;
  if (optrs.has_value()) grouped_check_table(*optrs, dy, Ne, at::kLong, name, "optrs");
  else out = at::empty({Ne, N, K}, dy.options().dtype(at::kFloat));
  grouped_gemm_wgrad(cptr<bf16_t>(dy), cptr<bf16_t>(x), cptr<int32_t>(offsets), optr<int64_t>(optrs),
                     out.has_value() ? ptr<float>(*out) : nullptr, R, N, K, (int)Ne, accumulate, cur_stream(dy));
  return out;
}

// xe [nslots, E]: xe[s] = x[src[s] / k], zeros for an empty slot.
Tensor py_moe_gather_slots(Tensor x, Tensor src, int64_t k) {
  const char* name = "moe_gather_slots";
  moe_check_rows(x, name, "x");
  MP_CHECK(k >= 1 && k <= 8, name, ": k must be in [1, 8], got ", k);
  const int64_t T = x.size(0), E = x.size(1), nslots = src.numel();
  moe_check_i32(src, x, nslots, name, "src");
  MP_CHECK(T * k < (int64_t(1) << 31) && nslots < (int64_t(1) << 31), name, ": T * k and the slots must be below 2^31");
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto xe = at::empty({nslots, E}, x.options());
  auto s = cur_stream(x);
  dispatch_fb(x, name, [&](auto* tag) {
    using T_ = std::remove_pointer_t<decltype(tag)>;
    moe_gather_slots<T_>(cptr<T_>(x), cptr<int32_t>(src), ptr<T_>(xe), nslots, T, (int)k, (int)E, s);
  });
  return xe;
}

// y [T, E]: y[t] = res[t] + sum_j w[t, j] ye[slot[t, j]] (w fp32 [T, k] and res [T, E] optional).
Tensor py_moe_gather_tokens(Tensor ye, Tensor slot, std::optional<Tensor> w, std::optional<Tensor> res) {
  const char* name = "moe_gather_tokens";
  moe_check_rows(ye, name, "ye");
  check_cuda(slot, "slot");
  MP_CHECK(slot.dim() == 2 && slot.size(1) >= 1 && slot.size(1) <= 8, name, ": slot must be [T, k] with k in [1, 8]");
  const int64_t T = slot.size(0), k = slot.size(1), nslots = ye.size(0), E = ye.size(1);
  moe_check_i32(slot, ye, T * k, name, "slot");
  MP_CHECK(nslots < (int64_t(1) << 31), name, ": the slots must be below 2^31");
  if (w.has_value()) moe_check_f32(*w, ye, T * k, name, "w");
  if (res.has_value()) {
    moe_check_rows(*res, name, "res");
    check_same(ye, *res, "ye", "res");
    MP_CHECK(res->size(0) == T && res->size(1) == E, name, ": res must be [T, E]");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(ye.device());
  auto y = at::empty({T, E}, ye.options());
  auto s = cur_stream(ye);
  dispatch_fb(ye, name, [&](auto* tag) {
    using T_ = std::remove_pointer_t<decltype(tag)>;
    moe_gather_tokens<T_>(cptr<T_>(ye), cptr<int32_t>(slot), optr<float>(w), optr<T_>(res), ptr<T_>(y), T, (int)k,
                          nslots, (int)E, s);
  });
  return y;
}

// (dye [nslots, E], dgate fp32 [T, k]) of dy [T, E], ye [nslots, E], gate [T, k], src [nslots].
std::tuple<Tensor, Tensor> py_moe_combine_bwd(Tensor dy, Tensor ye, Tensor gate, Tensor src) {
  const char* name = "moe_combine_bwd";
  moe_check_rows(dy, name, "dy");
  moe_check_rows(ye, name, "ye");
  check_same(dy, ye, "dy", "ye");
  check_cuda(gate, "gate");
  MP_CHECK(gate.dim() == 2 && gate.size(0) == dy.size(0) && gate.size(1) >= 1 && gate.size(1) <= 8, name,
           ": gate must be [T, k] with k in [1, 8]");
  const int64_t T = dy.size(0), E = dy.size(1), k = gate.size(1), nslots = ye.size(0);
  MP_CHECK(ye.size(1) == E, name, ": dy and ye must have the same width");
  moe_check_f32(gate, dy, T * k, name, "gate");
  moe_check_i32(src, dy, nslots, name, "src");
  MP_CHECK(T * k < (int64_t(1) << 31) && nslots < (int64_t(1) << 31), name, ": T * k and the slots must be below 2^31");
  at::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
  auto dye = at::empty_like(ye);
  auto dgate = at::zeros({T, k}, gate.options());  // a dropped (t, j) keeps its 0
  auto s = cur_stream(dy);
  dispatch_fb(dy, name, [&](auto* tag) {
    using T_ = std::remove_pointer_t<decltype(tag)>;
    moe_combine_bwd<T_>(cptr<T_>(dy), cptr<T_>(ye), cptr<float>(gate), cptr<int32_t>(src), ptr<T_>(dye),
                        ptr<float>(dgate), nslots, T, (int)k, (int)E, s);
  });
  return {dye, dgate};
}

// dkv [B, S, 2, H, D] (per-query-head dK / dV partials) summed per group into the K and V heads of
// dqkv [B, S, H + 2 Hkv, D]; the Q heads of dqkv are not touched.
void py_gqa_reduce_dkv(Tensor dkv, Tensor dqkv, int64_t H, int64_t Hkv) {
  check_cuda(dkv, "dkv");
  check_cuda(dqkv, "dqkv");
  check_same(dkv, dqkv, "dkv", "dqkv");
  MP_CHECK(H > 0 && Hkv > 0 && H % Hkv == 0, "gqa_reduce_dkv: H must be a positive multiple of Hkv, got ", H, " / ", Hkv);
  MP_CHECK(dkv.dim() == 5 && dkv.size(2) == 2 && dkv.size(3) == H, "gqa_reduce_dkv: dkv must be [B, S, 2, H, D]");
  const int64_t B = dkv.size(0), S = dkv.size(1), D = dkv.size(4);
  MP_CHECK(D > 0 && D % 8 == 0, "gqa_reduce_dkv: head dim must be a multiple of 8, got ", D);
  MP_CHECK(dqkv.dim() == 4 && dqkv.size(0) == B && dqkv.size(1) == S && dqkv.size(2) == H + 2 * Hkv &&
               dqkv.size(3) == D,
           "gqa_reduce_dkv: dqkv must be [B, S, H + 2 Hkv, D] = [", B, ", ", S, ", ", H + 2 * Hkv, ", ", D, "]");
  MP_CHECK(dkv.is_contiguous() && dqkv.is_contiguous(), "gqa_reduce_dkv: dkv and dqkv must be contiguous");
  MP_CHECK(H * D <= INT32_MAX / 8, "gqa_reduce_dkv: shape too large");
  at::hip::HIPGuardMasqueradingAsCUDA guard(dkv.device());
  auto s = cur_stream(dkv);
  dispatch_fb(dkv, "gqa_reduce_dkv", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    gqa_reduce_dkv<T>(cptr<T>(dkv), ptr<T>(dqkv), B * S, (int)H, (int)Hkv, (int)D, s);
  });
}

std::tuple<Tensor, int64_t, int64_t> py_bias_act_fwd(Tensor x, std::optional<Tensor> bias, int64_t act, double p) {
  check_cuda(x, "x");
  const int64_t cols = x.size(-1);
  const int64_t rows = x.numel() / std::max<int64_t>(cols, 1);
  MP_CHECK(cols % 8 == 0, "bias_act: last dim must be a multiple of 8");
  MP_CHECK(act >= 0 && act <= 2, "bias_act: bad activation");
  MP_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1)");
  if (bias) {
    check_cuda(*bias, "bias");
    check_same(x, *bias, "x", "bias");
    MP_CHECK(bias->numel() == cols, "bias_act: bias size mismatch");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty_like(x);
  uint64_t seed = 0, offset = 0;
  if (p > 0.0) std::tie(seed, offset) = philox_draw(x.device(), 4);
  auto s = cur_stream(x);
  dispatch_fb(x, "bias_act_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    bias_act_dropout_fwd<T>(cptr<T>(x), optr<T>(bias), ptr<T>(y), rows, (int)cols, (int)act, (float)p, seed, offset, s);
  });
  return {y, (int64_t)seed, (int64_t)offset};
}

Tensor py_column_sum(Tensor x, std::optional<Tensor> out, bool accumulate);

// Logit soft-capping.  A tensor is read as rows of its last dim: unit stride there, and leading dims that
// collapse to one row stride (a contiguous tensor, or the [:, :V] view of a padded one).
struct RowView { int64_t rows = 1, cols = 0, ld = 0; };
RowView softcap_rows(const Tensor& t, const char* who, const char* name) {
  RowView r;
  if (t.dim() == 0) { r.cols = 1; r.ld = 1; return r; }
  const int64_t n = t.dim();
  r.cols = t.size(n - 1);
  r.ld = r.cols;
  MP_CHECK(r.cols <= 1 || t.stride(n - 1) == 1, who, ": ", name, " needs unit stride on its last dim");
  if (n >= 2) {
    r.ld = t.stride(n - 2);
    r.rows = t.size(n - 2);
    MP_CHECK(r.rows <= 1 || r.ld >= r.cols, who, ": ", name, " has overlapping rows");
    for (int64_t i = n - 3; i >= 0; --i) {
      MP_CHECK(t.size(i) <= 1 || t.stride(i) == t.stride(i + 1) * t.size(i + 1), who, ": ", name,
               " must have one row stride (make it contiguous)");
      r.rows *= t.size(i);
    }
  }
  return r;
}

float softcap_cap(const char* who, double cap) {
  const float c = (float)cap;
  MP_CHECK(std::isfinite(cap) && cap > 0.0 && std::isfinite(c) && c > 0.f, who, ": cap must be a finite value > 0, got ",
           cap);
  return c;
}

// y = cap * tanh(x / cap); `out` (x itself for the in-place form) or a new contiguous tensor.
Tensor py_softcap_fwd(Tensor x, double cap, std::optional<Tensor> out) {
  MP_CHECK(x.is_cuda(), "softcap: x must be a GPU tensor");
  const float c = softcap_cap("softcap", cap);
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out ? *out : at::empty(x.sizes(), x.options());
  if (out) {
    MP_CHECK(y.is_cuda(), "softcap: out must be a GPU tensor");
    check_same(x, y, "x", "out");
    MP_CHECK(y.sizes() == x.sizes(), "softcap: out must have x's shape");
  }
  const RowView rx = softcap_rows(x, "softcap", "x"), ry = softcap_rows(y, "softcap", "out");
  auto s = cur_stream(x);
  dispatch_fb(x, "softcap", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    softcap_fwd<T>(cptr<T>(x), rx.ld, ptr<T>(y), ry.ld, rx.rows, rx.cols, c, s);
  });
  return y;
}

// dx = dy * (1 - (y / cap)^2) from the saved output y; `out` (dy itself for the in-place form) or a new tensor.
Tensor py_softcap_bwd(Tensor dy, Tensor y, double cap, std::optional<Tensor> out) {
  MP_CHECK(dy.is_cuda(), "softcap: dy must be a GPU tensor");
  MP_CHECK(y.is_cuda(), "softcap: y must be a GPU tensor");
  check_same(dy, y, "dy", "y");
  MP_CHECK(dy.sizes() == y.sizes(), "softcap_bwd: dy and y shapes differ");
  const float c = softcap_cap("softcap_bwd", cap);
  at::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
  Tensor dx = out ? *out : at::empty(dy.sizes(), dy.options());
  if (out) {
    MP_CHECK(dx.is_cuda(), "softcap: out must be a GPU tensor");
    check_same(dy, dx, "dy", "out");
    MP_CHECK(dx.sizes() == dy.sizes(), "softcap_bwd: out must have dy's shape");
  }
  const RowView rd = softcap_rows(dy, "softcap_bwd", "dy"), ry = softcap_rows(y, "softcap_bwd", "y"),
                ro = softcap_rows(dx, "softcap_bwd", "out");
  auto s = cur_stream(dy);
  dispatch_fb(dy, "softcap_bwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    softcap_bwd<T>(cptr<T>(dy), rd.ld, cptr<T>(y), ry.ld, ptr<T>(dx), ro.ld, rd.rows, rd.cols, c, s);
  });
  return dx;
}

std::tuple<Tensor, std::optional<Tensor>> py_bias_act_bwd(Tensor dy, Tensor saved, std::optional<Tensor> bias,
                                                          int64_t act, double p, int64_t seed, int64_t offset,
                                                          bool need_dbias, std::optional<Tensor> dbias_acc) {
  check_cuda(dy, "dy");
  check_cuda(saved, "saved");
  check_same(dy, saved, "dy", "saved");
  MP_CHECK(dy.numel() == saved.numel(), "bias_act_bwd: shape mismatch");
  const int64_t cols = dy.size(-1);
  const int64_t rows = dy.numel() / std::max<int64_t>(cols, 1);
  MP_CHECK(cols % 8 == 0, "bias_act_bwd: last dim must be a multiple of 8");
  if (bias) MP_CHECK(bias->numel() == cols, "bias_act_bwd: bias size mismatch");
  at::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
  auto dx = at::empty_like(dy);
  auto s = cur_stream(dy);
  dispatch_fb(dy, "bias_act_bwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    bias_act_dropout_bwd<T>(cptr<T>(dy), cptr<T>(saved), optr<T>(bias), ptr<T>(dx), rows, (int)cols, (int)act,
                            (float)p, (uint64_t)seed, (uint64_t)offset, s);
  });
  std::optional<Tensor> db;
  if (dbias_acc.has_value()) {
    py_column_sum(dx.view({rows, cols}), dbias_acc, true);  // fp32 main_grad += colsum
  } else if (need_dbias) {
    db = py_column_sum(dx.view({rows, cols}), std::nullopt, false);
  }
  return {dx, db};
}

Tensor py_column_sum(Tensor x, std::optional<Tensor> out, bool accumulate) {
  check_cuda(x, "x");
  const int64_t cols = x.size(-1);
  const int64_t rows = x.numel() / std::max<int64_t>(cols, 1);
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor o = out.has_value() ? *out : at::empty({cols}, x.options());
  MP_CHECK(o.numel() == cols && o.is_contiguous(), "column_sum: bad out");
  const bool out_f32 = o.scalar_type() == at::kFloat;
  MP_CHECK(out_f32 || o.scalar_type() == x.scalar_type(), "column_sum: out must be fp32 or the input dtype");
  if (rows == 0) {
    if (!accumulate) o.zero_();
    return o;
  }
  const int nparts = colsum_parts(rows, cols);
  auto part = at::empty({nparts, cols}, x.options().dtype(at::kFloat));
  auto s = cur_stream(x);
  dispatch_fb(x, "column_sum", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    column_sum<T>(cptr<T>(x), rows, (int)cols, ptr<float>(part), nparts, o.data_ptr(), out_f32, accumulate, s);
  });
  return o;
}

// ------------------------------------------------------------------ cross entropy
void check_rows(const Tensor& t, const char* name) {
  MP_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  MP_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) >= t.size(1), name, " must be 2-D with unit column stride");
}

std::tuple<Tensor, Tensor> py_ce_fwd(Tensor logits, Tensor target, int64_t ignore_index, int64_t t_offset) {
  check_rows(logits, "logits");
  check_cuda(target, "target");
  MP_CHECK(target.scalar_type() == at::kLong && target.is_contiguous(), "cross_entropy: target must be contiguous int64");
  MP_CHECK(logits.dim() == 2 && target.numel() == logits.size(0), "cross_entropy: expects [N, V] logits and [N] target");
  at::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  const int64_t rows = logits.size(0), V = logits.size(1);
  auto fopt = logits.options().dtype(at::kFloat);
  auto loss = at::empty({rows}, fopt);
  auto lse = at::empty({rows}, fopt);
  auto s = cur_stream(logits);
  dispatch_fb(logits, "cross_entropy_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    cross_entropy_fwd<T>(cptr<T>(logits), cptr<int64_t>(target), rows, V, logits.stride(0), ignore_index,
                         ptr<float>(loss), ptr<float>(lse), s, t_offset);
  });
  return {loss, lse};
}

// Mean cross-entropy over the valid targets: (loss [] fp32, lse [N], weight [N] = valid / count).
std::tuple<Tensor, Tensor, Tensor> py_ce_mean_fwd(Tensor logits, Tensor target, int64_t ignore_index) {
  check_rows(logits, "logits");
  check_cuda(target, "target");
  MP_CHECK(target.scalar_type() == at::kLong && target.numel() == logits.size(0),
           "cross_entropy_mean: expects [N, V] logits and [N] int64 target");
  at::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  const int64_t rows = logits.size(0), V = logits.size(1);
  auto fopt = logits.options().dtype(at::kFloat);
  auto loss_row = at::empty({rows}, fopt);
  auto lse = at::empty({rows}, fopt);
  auto weight = at::empty({rows}, fopt);
  auto loss = at::empty({}, fopt);
  auto s = cur_stream(logits);
  dispatch_fb(logits, "cross_entropy_mean_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    cross_entropy_mean_fwd<T>(cptr<T>(logits), cptr<int64_t>(target), rows, V, logits.stride(0), ignore_index,
                              ptr<float>(loss_row), ptr<float>(lse), ptr<float>(weight), ptr<float>(loss), s);
  });
  return {loss, lse, weight};
}

// A per-row fp32 vector, possibly strided (a column of a packed message's
// statistic slots): its stride in floats.
int64_t row_vector(const Tensor& t, int64_t rows, const char* name) {
  MP_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.dim() == 1 && t.size(0) == rows, name,
           " must be a [rows] fp32 GPU tensor");
  return rows > 1 ? t.stride(0) : 1;
}

// The statistic slots of a packed split-decoder message: `slots` is the
// [rows, n] column slice after the hidden values, in the activation dtype.
// Returns (fp32 word pointer, row stride in words, words per row).
std::tuple<float*, int64_t, int> stat_slots(const Tensor& slots, int64_t rows, const char* name) {
  MP_CHECK(slots.is_cuda(), name, " must be a GPU tensor");
  MP_CHECK(slots.dim() == 2 && slots.size(0) == rows && slots.stride(1) == 1, name, " must be [rows, n] with unit column stride");
  const int64_t es = slots.element_size();
  const int64_t ld = rows > 1 ? slots.stride(0) : slots.size(1);
  MP_CHECK((ld * es) % 4 == 0 && (slots.size(1) * es) % 4 == 0 && reinterpret_cast<uintptr_t>(slots.data_ptr()) % 4 == 0,
           name, ": slots must hold whole, aligned fp32 words");
  const int nslot = (int)(slots.size(1) * es / 4);
  MP_CHECK(nslot >= 2 && nslot <= 256, name, ": need 2..256 fp32 words per row");
  return {reinterpret_cast<float*>(slots.data_ptr()), ld * es / 4, nslot};
}

// out (optional): [N, >= V] destination with unit column stride (e.g. a
// zero-padded vocabulary buffer); row_scale (optional): per-row scale, see loss.hip.
// zero_pad: columns [V, out.size(1)) of `out` are zeroed (padded-vocabulary gradient).
// lse / row_scale may be strided; scale and row_scale together multiply.
// stat_out (optional): [N, n] slots receiving (lse, row scale) (split decoder).
Tensor py_ce_bwd(Tensor logits, Tensor target, Tensor lse, std::optional<Tensor> scale, int64_t ignore_index,
                 std::optional<Tensor> row_scale, std::optional<Tensor> out, bool zero_pad, int64_t t_offset,
                 std::optional<Tensor> stat_out) {
  check_rows(logits, "logits");
  const int64_t rows = logits.size(0);
  check_cuda(target, "target");
  MP_CHECK(target.scalar_type() == at::kLong && target.is_contiguous() && target.numel() == rows,
           "cross_entropy_bwd: target must be contiguous int64 [N]");
  const int64_t ld_lse = row_vector(lse, rows, "lse");
  MP_CHECK(scale.has_value() || row_scale.has_value(), "cross_entropy_bwd: give scale and/or row_scale");
  if (scale)
    MP_CHECK(scale->scalar_type() == at::kFloat && scale->numel() == 1 && scale->is_cuda(), "cross_entropy_bwd: bad scale");
  const int64_t ld_rs = row_scale ? row_vector(*row_scale, rows, "row_scale") : 1;
  at::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  Tensor d;
  if (out) {
    MP_CHECK(out->dim() == 2 && out->size(0) == rows && out->size(1) >= logits.size(1) &&
                 out->stride(1) == 1 && out->scalar_type() == logits.scalar_type() && out->is_cuda(),
             "cross_entropy_bwd: bad out");
    d = *out;
  } else {
    d = at::empty({rows, logits.size(1)}, logits.options());
  }
  float* st = nullptr;
  int64_t ld_st = 0;
  int nslot = 0;
  if (stat_out) std::tie(st, ld_st, nslot) = stat_slots(*stat_out, rows, "stat_out");
  auto s = cur_stream(logits);
  dispatch_fb(logits, "cross_entropy_bwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    cross_entropy_bwd<T>(cptr<T>(logits), cptr<int64_t>(target), cptr<float>(lse),
                         scale ? cptr<float>(*scale) : nullptr, row_scale ? cptr<float>(*row_scale) : nullptr,
                         rows, logits.size(1), logits.stride(0), d.stride(0), ignore_index, ptr<T>(d),
                         zero_pad ? d.size(1) : logits.size(1), s, t_offset, ld_lse, ld_rs, st, ld_st, nslot);
  });
  return d;
}

// Split-decoder head forward (mipipe/models/vocab_split.py): packs x into
// out[:, :E] and (lse, target logit) into the slots out[:, E:].
void py_vsplit_head_fwd(Tensor logits, Tensor target, Tensor x, Tensor out) {
  check_rows(logits, "logits");
  check_rows(x, "x");
  check_rows(out, "out");
  const int64_t rows = logits.size(0), E = x.size(1);
  MP_CHECK(x.size(0) == rows && out.size(0) == rows && out.size(1) > E, "vsplit_head_fwd: shape mismatch");
  MP_CHECK(x.scalar_type() == logits.scalar_type() && out.scalar_type() == x.scalar_type(), "vsplit_head_fwd: dtypes differ");
  MP_CHECK(target.is_cuda() && target.scalar_type() == at::kLong && target.is_contiguous() && target.numel() == rows,
           "vsplit_head_fwd: target must be contiguous int64 [N]");
  const int64_t es = x.element_size();
  MP_CHECK((E * es) % 16 == 0 && (x.stride(0) * es) % 16 == 0 && (out.stride(0) * es) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
           "vsplit_head_fwd: x / out rows must be 16-byte aligned");
  auto [st, ld_st, nslot] = stat_slots(out.narrow(1, E, out.size(1) - E), rows, "out slots");
  (void)st;
  (void)ld_st;
  at::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  auto s = cur_stream(logits);
  dispatch_fb(logits, "vsplit_head_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    vsplit_head_fwd<T>(cptr<T>(logits), logits.stride(0), rows, logits.size(1), cptr<int64_t>(target), cptr<T>(x),
                       x.stride(0), E, ptr<T>(out), out.stride(0), nslot, s);
  });
}

// Split-decoder tail forward: returns (loss [] fp32, lse [N], weight [N] = valid / count).
std::tuple<Tensor, Tensor, Tensor> py_vsplit_tail_fwd(Tensor logits, Tensor target, int64_t t_offset,
                                                      int64_t ignore_index, Tensor slots) {
  check_rows(logits, "logits");
  const int64_t rows = logits.size(0);
  MP_CHECK(target.is_cuda() && target.scalar_type() == at::kLong && target.is_contiguous() && target.numel() == rows,
           "vsplit_tail_fwd: target must be contiguous int64 [N]");
  auto [st, ld_st, nslot] = stat_slots(slots, rows, "slots");
  (void)nslot;
  at::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  auto fopt = logits.options().dtype(at::kFloat);
  auto loss = at::empty({}, fopt);
  auto lse = at::empty({rows}, fopt);
  auto loss_row = at::empty({rows}, fopt);
  auto weight = at::empty({rows}, fopt);
  auto s = cur_stream(logits);
  dispatch_fb(logits, "vsplit_tail_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    vsplit_tail_fwd<T>(cptr<T>(logits), logits.stride(0), rows, logits.size(1), cptr<int64_t>(target), t_offset,
                       ignore_index, st, ld_st, ptr<float>(lse), ptr<float>(loss_row), ptr<float>(weight),
                       ptr<float>(loss), s);
  });
  return {loss, lse, weight};
}

// ------------------------------------------------------------------ embedding
std::tuple<Tensor, int64_t, int64_t> py_embed_fwd(Tensor tokens, Tensor weight, std::optional<Tensor> pe,
                                                  double scale, double p) {
  check_cuda(tokens, "tokens");
  check_cuda(weight, "weight");
  MP_CHECK(tokens.scalar_type() == at::kLong && tokens.dim() == 2, "embedding: tokens must be int64 [B, S]");
  MP_CHECK(weight.dim() == 2 && weight.size(1) % 8 == 0, "embedding: weight must be [V, E] with E % 8 == 0");
  const int64_t S = tokens.size(1), E = weight.size(1), V = weight.size(0);
  if (pe) {
    check_cuda(*pe, "pe");
    MP_CHECK((pe->scalar_type() == at::kFloat || pe->scalar_type() == weight.scalar_type()) && pe->dim() == 2 &&
                 pe->size(1) == E && pe->size(0) >= S && pe->is_contiguous(),
             "embedding: pe must be a contiguous fp32 or weight-dtype [max_len >= S, E]");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(weight.device());
  auto out = at::empty({tokens.size(0), S, E}, weight.options());
  uint64_t seed = 0, offset = 0;
  if (p > 0.0) std::tie(seed, offset) = philox_draw(weight.device(), 4);
  auto s = cur_stream(weight);
  dispatch_fb(weight, "embedding_fwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    embedding_fwd<T>(cptr<int64_t>(tokens), cptr<T>(weight), pe ? pe->data_ptr() : nullptr,
                     pe ? pe->scalar_type() == at::kFloat : true, ptr<T>(out), tokens.numel(), (int)S, (int)E, V,
                     (float)scale, (float)p, seed, offset, s);
  });
  return {out, (int64_t)seed, (int64_t)offset};
}

// dpe (optional): fp32 [max_len, E] gradient of a learned position table, accumulated.
void py_embed_bwd(Tensor tokens, Tensor dout, Tensor dweight, double scale, double p, int64_t seed, int64_t offset,
                  std::optional<Tensor> dpe) {
  check_cuda(dout, "dout");
  check_cuda(dweight, "dweight");
  check_cuda(tokens, "tokens");
  MP_CHECK(tokens.scalar_type() == at::kLong && tokens.dim() == 2, "embedding_bwd: tokens must be int64 [B, S]");
  MP_CHECK(dweight.scalar_type() == at::kFloat && dweight.dim() == 2, "embedding_bwd: dweight must be fp32 [V, E]");
  const int64_t E = dweight.size(1), V = dweight.size(0);
  MP_CHECK(dout.numel() == tokens.numel() * E, "embedding_bwd: shape mismatch");
  MP_CHECK(E % 8 == 0 && E <= 8192, "embedding_bwd: E must be a multiple of 8 and at most 8192");
  if (dpe) {
    check_cuda(*dpe, "dpe");
    MP_CHECK(dpe->scalar_type() == at::kFloat && dpe->dim() == 2 && dpe->size(1) == E &&
                 dpe->size(0) >= tokens.size(1), "embedding_bwd: dpe must be fp32 [>= S, E]");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(dout.device());
  auto s = cur_stream(dout);
  dispatch_fb(dout, "embedding_bwd", [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    embedding_bwd<T>(cptr<int64_t>(tokens), cptr<T>(dout), ptr<float>(dweight), tokens.numel(), (int)E, V,
                     (float)scale, (float)p, (uint64_t)seed, (uint64_t)offset, s, dpe ? ptr<float>(*dpe) : nullptr,
                     (int)tokens.size(1));
  });
}

// ------------------------------------------------------------------ GEMM
// GEMM operands: bf16 (v_mfma_f32_16x16x32_bf16 kernel) or fp32 (v_mfma_f32_32x32x2_f32 kernel).
// Layout (unit column stride, aligned row stride) is checked by row_stride().
void check_gemm_2d(const Tensor& t, const char* name) {
  MP_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  MP_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat, name, " must be bf16 or fp32");
  MP_CHECK(t.dim() == 2, name, " must be 2-D");
  MP_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

// Row stride of a 2-D GEMM operand / output: unit column stride and 16-byte
// aligned rows (the tile kernels move 16-byte chunks), so row-strided views
// -- a column slice of a packed activation -- need no copy.
int64_t row_stride(const Tensor& t, const char* name) {
  MP_CHECK(t.dim() == 2 && (t.stride(1) == 1 || t.size(1) == 1), name, " must have unit column stride");
  const int64_t ld = t.size(0) > 1 ? t.stride(0) : t.size(1);
  MP_CHECK(ld >= t.size(1) && (ld * (int64_t)t.element_size()) % 16 == 0, name,
           ": rows must be 16-byte aligned (row stride ", ld, ")");
  return ld;
}

void check_same_dtype(const Tensor& a, const Tensor& b, const char* what) {
  MP_CHECK(a.scalar_type() == b.scalar_type(), what, ": operand dtypes differ");
}

bool gemm_ok(at::ScalarType t, int64_t M, int64_t N, int64_t K) {
  return t == at::kFloat ? gemm_f32_supported(M, N, K) : gemm_supported(M, N, K);
}

void gemm_run(at::ScalarType t, const GemmArgs& g, hipStream_t s) {
  if (t == at::kFloat) gemm_f32(g, s);
  else gemm_bf16(g, s);
}

// y[M,N] = act(x[M,K] . w[N,K]^T + bias) with dropout; optional pre-activation.
// xt (optional, bf16 [K, M]): also written with x^T by the same GEMM (its
// blocks transpose the x tiles they stage anyway), the K-contiguous operand of
// the layer's transposed weight-gradient GEMM (linear_wgrad_xt_segments).
std::tuple<Tensor, std::optional<Tensor>, int64_t, int64_t> py_linear_fwd(Tensor x, Tensor w,
                                                                           std::optional<Tensor> bias, int64_t act,
                                                                           double p, bool save_preact,
                                                                           std::optional<Tensor> res,
                                                                           std::optional<Tensor> xt,
                                                                           bool aux_grad,
                                                                           std::optional<Tensor> bits) {
  check_gemm_2d(x, "x");
  check_gemm_2d(w, "w");
  check_same_dtype(x, w, "linear_fwd");
  const auto dt = x.scalar_type();
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  MP_CHECK(w.size(1) == K, "linear_fwd: inner dims differ");
  MP_CHECK(gemm_ok(dt, M, N, K), "linear_fwd: unsupported shape ", M, "x", N, "x", K);
  MP_CHECK(act >= 0 && act <= 2 && p >= 0.0 && p < 1.0, "linear_fwd: bad act/p");
  MP_CHECK(!aux_grad || (act == kActGelu && save_preact && dt == at::kBFloat16),
           "linear_fwd: aux_grad (GELU'(pre) as the saved tensor) needs bf16, GELU and save_preact");
  if (bias) {
    check_cuda(*bias, "bias");
    MP_CHECK(bias->scalar_type() == dt && bias->numel() == N, "linear_fwd: bad bias");
  }
  if (res) {
    check_gemm_2d(*res, "res");
    check_same_dtype(x, *res, "linear_fwd res");
    MP_CHECK(res->size(0) == M && res->size(1) == N, "linear_fwd: res must be [M, N]");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({M, N}, x.options());
  std::optional<Tensor> pre;
  if (save_preact) pre = at::empty({M, N}, x.options());
  uint64_t seed = 0, offset = 0;
  if (p > 0.0) std::tie(seed, offset) = philox_draw(x.device(), 4);
  GemmArgs g;
  g.A = x.data_ptr(); g.B = w.data_ptr(); g.C = y.data_ptr();
  g.bias = bias ? bias->data_ptr() : nullptr; g.aux = pre ? pre->data_ptr() : nullptr;
  g.aux_grad = aux_grad;
  if (res) {
    g.res = res->data_ptr();  // y = res + dropout(act(x . w^T + b)): the residual add in the epilogue
    g.ldr = row_stride(*res, "res");
  }
  g.lda = row_stride(x, "x"); g.ldb = row_stride(w, "w"); g.ldc = N; g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.a_kc = true; g.b_kc = true; g.epi = kEpiStoreAct; g.act = (int)act; g.p = (float)p;
  g.seed = seed; g.offset = offset;
  if (xt) {
    check_gemm_2d(*xt, "xt");
    MP_CHECK(dt == at::kBFloat16 && xt->scalar_type() == dt && xt->size(0) == K && xt->size(1) == M,
             "linear_fwd: xt must be bf16 [K, M]");
    MP_CHECK(gemm_emit_ok((int)act, (float)p, save_preact), "linear_fwd: this epilogue cannot write xt (gemm_emit_ok)");
    g.at = xt->data_ptr();
    g.ldat = row_stride(*xt, "xt");
  }
  if (bits) {  // the output's nonzero mask as bits, for the consumer's dgrad (kActReluBits)
    check_cuda(*bits, "bits");
    MP_CHECK(bits->scalar_type() == at::kByte && bits->dim() == 2 && bits->size(0) == M && bits->size(1) * 8 == N &&
                 bits->stride(1) == 1,
             "linear_fwd: bits must be uint8 [M, N / 8] with unit column stride");
    g.bits = bits->data_ptr();
    g.ldbits = bits->stride(0);
    MP_CHECK(dt == at::kBFloat16 && gemm_plan(g).bits_ok, "linear_fwd: this launch cannot write bits (GemmPlan::bits_ok)");
  }
  gemm_run(dt, g, cur_stream(x));
  return {y, pre, (int64_t)seed, (int64_t)offset};
}

// Split-K (bf16 GEMMs on under-filled grids, GemmPlan::k_splits): the fp32
// partials' workspace, from the stream-ordered caching allocator (released
// after the kernels queued on this stream that use it).  Empty when unsplit.
Tensor split_k_workspace(GemmArgs& g, at::ScalarType dt, const Tensor& like) {
  if (dt != at::kBFloat16) return Tensor();
  const int splits = gemm_plan(g).k_splits;
  if (splits <= 1) return Tensor();
  Tensor ws = at::empty({splits, (int64_t)g.M, (int64_t)g.N}, like.options().dtype(at::kFloat));
  g.k_splits = splits;
  g.ws = ws.data_ptr<float>();
  return ws;
}

// dx[M,K] = dy[M,N] . w[N,K]
// dx = dy . w (+ res): `res` is the gradient the input receives from its
// other consumer (a residual branch), added in the epilogue.
// act (optional, with `saved`): the output is the gradient of the activation's
// INPUT -- act'(saved) (and the forward's dropout mask: p, seed, offset) applied
// in the epilogue (GELU: saved = the pre-activation; ReLU: saved = the output).
Tensor py_linear_dgrad(Tensor dy, Tensor w, std::optional<Tensor> res, std::optional<Tensor> out, int64_t act,
                       std::optional<Tensor> saved, double p, int64_t seed, int64_t offset) {
  check_gemm_2d(dy, "dy");
  check_gemm_2d(w, "w");
  check_same_dtype(dy, w, "linear_dgrad");
  const auto dt = dy.scalar_type();
  const int64_t M = dy.size(0), N = dy.size(1), K = w.size(1);
  MP_CHECK(w.size(0) == N, "linear_dgrad: inner dims differ");
  MP_CHECK(gemm_ok(dt, M, K, N), "linear_dgrad: unsupported shape");
  if (res) {
    check_gemm_2d(*res, "res");
    check_same_dtype(dy, *res, "linear_dgrad res");
    MP_CHECK(res->size(0) == M && res->size(1) == K, "linear_dgrad: res must be [M, K]");
  }
  MP_CHECK(act == kActNone || act == kActRelu || act == kActGelu || act == kActSavedGrad || act == kActReluBits,
           "linear_dgrad: bad act");
  if (act != kActNone) {
    // (with `res`: dx = (dy . w) x act'(saved) + res, the order of the GEMM's store pass)
    MP_CHECK(saved.has_value() && dt == at::kBFloat16, "linear_dgrad: the activation backward needs bf16 "
             "operands and the saved tensor");
    if (act == kActReluBits) {
      check_cuda(*saved, "saved");
      MP_CHECK(saved->scalar_type() == at::kByte && saved->dim() == 2 && saved->size(0) == M &&
                   saved->size(1) * 8 == K && saved->stride(1) == 1,
               "linear_dgrad: the ReLU bit mask must be uint8 [M, K / 8] with unit column stride");
    } else {
      check_gemm_2d(*saved, "saved");
      check_same_dtype(dy, *saved, "linear_dgrad saved");
      MP_CHECK(saved->size(0) == M && saved->size(1) == K, "linear_dgrad: saved must be [M, K]");
    }
    MP_CHECK(p >= 0.0 && p < 1.0, "linear_dgrad: bad p");
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
  Tensor dx;
  if (out) {  // a (row-strided) destination, e.g. the columns of a packed gradient message
    check_gemm_2d(*out, "out");
    MP_CHECK(out->size(0) == M && out->size(1) == K && out->scalar_type() == dt, "linear_dgrad: bad out");
    dx = *out;
  } else {
    dx = at::empty({M, K}, dy.options());
  }
  GemmArgs g;
  g.A = dy.data_ptr(); g.B = w.data_ptr(); g.C = dx.data_ptr();
  if (res) {
    g.res = res->data_ptr();
    g.ldr = row_stride(*res, "res");
  }
  g.lda = row_stride(dy, "dy"); g.ldb = row_stride(w, "w"); g.ldc = row_stride(dx, "out");
  g.M = (int)M; g.N = (int)K; g.K = (int)N;
  g.a_kc = true; g.b_kc = false; g.epi = kEpiStoreAct;
  if (act != kActNone) {
    g.dact_in = saved->data_ptr();
    g.ldd = act == kActReluBits ? saved->stride(0) : row_stride(*saved, "saved");
    g.dact = (int)act;
    if (act == kActRelu || act == kActReluBits) {  // the saved output's sign (or its bit) is the mask as well
      g.dact_scale = p > 0.0 ? (float)(1.0 / (1.0 - p)) : 1.f;
    } else {
      g.p = (float)p;
      g.seed = (uint64_t)seed;
      g.offset = (uint64_t)offset;
    }
  }
  Tensor ws = split_k_workspace(g, dt, dy);
  gemm_run(dt, g, cur_stream(dy));
  return dx;
}

// main_grad[N,K] (fp32) += dy[T,N]^T . x[T,K]   (= when !accumulate)
void py_linear_wgrad(Tensor dy, Tensor x, Tensor main_grad, bool accumulate) {
  check_gemm_2d(dy, "dy");
  check_gemm_2d(x, "x");
  check_same_dtype(dy, x, "linear_wgrad");
  const auto dt = dy.scalar_type();
  check_cuda(main_grad, "main_grad");
  const int64_t T = dy.size(0), N = dy.size(1), K = x.size(1);
  MP_CHECK(x.size(0) == T, "linear_wgrad: token dims differ");
  MP_CHECK(main_grad.scalar_type() == at::kFloat && main_grad.numel() == N * K, "linear_wgrad: bad main_grad");
  MP_CHECK(gemm_ok(dt, N, K, T), "linear_wgrad: unsupported shape");
  at::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
  GemmArgs g;
  g.A = dy.data_ptr(); g.B = x.data_ptr(); g.C = main_grad.data_ptr();
  g.lda = row_stride(dy, "dy"); g.ldb = row_stride(x, "x"); g.ldc = K; g.M = (int)N; g.N = (int)K; g.K = (int)T;
  g.a_kc = false; g.b_kc = false; g.epi = accumulate ? kEpiAccumF32 : kEpiStoreF32;
  Tensor ws = split_k_workspace(g, dt, dy);
  gemm_run(dt, g, cur_stream(dy));
}

// Deferred bias gradient over the micro-batches of a step: out (+)= column sums
// of every [rows, cols] input, one stage-1 launch per input into a shared
// partial buffer and ONE reduction.
// x^T of a 2-D bf16/fp16 tensor [R, C] (row stride >= C, unit column stride)
// into a new contiguous [C, R] tensor: the K-contiguous operand of
// linear_wgrad_xt_segments when the flush transposes x itself (ops/linear.py).
Tensor py_transpose_b16(Tensor x) {
  MP_CHECK(x.is_cuda(), "x must be a GPU tensor");
  MP_CHECK(x.dim() == 2 && x.stride(1) == 1 && x.element_size() == 2, "transpose_b16: x must be 2-D, 2-byte, unit column stride");
  const int64_t R = x.size(0), C = x.size(1), ld = x.stride(0);
  MP_CHECK(R % 8 == 0 && C % 8 == 0 && ld % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
           "transpose_b16: rows, cols and row stride must be multiples of 8, x 16-byte aligned");
  MP_CHECK(C / 256 < 65536, "transpose_b16: too many columns");
  at::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto out = at::empty({C, R}, x.options());
  mipipe::transpose_b16(reinterpret_cast<const uint16_t*>(x.data_ptr()), R, C, ld,
                        reinterpret_cast<uint16_t*>(out.data_ptr()), R, cur_stream(x));
  return out;
}

void py_column_sum_segments(std::vector<Tensor> xs, Tensor out, bool accumulate) {
  MP_CHECK(!xs.empty(), "column_sum_segments: empty list");
  check_cuda(out, "out");
  const int64_t cols = xs[0].size(-1);
  MP_CHECK(out.numel() == cols && out.is_contiguous(), "column_sum_segments: bad out");
  const bool out_f32 = out.scalar_type() == at::kFloat;
  MP_CHECK(out_f32 || out.scalar_type() == xs[0].scalar_type(), "column_sum_segments: out must be fp32 or the input dtype");
  std::vector<int64_t> rows(xs.size());
  std::vector<int> parts(xs.size());
  int total = 0;
  for (size_t i = 0; i < xs.size(); ++i) {
    check_cuda(xs[i], "x");
    MP_CHECK(xs[i].is_contiguous() && xs[i].size(-1) == cols && xs[i].scalar_type() == xs[0].scalar_type(),
             "column_sum_segments: inputs must be contiguous with equal width and dtype");
    rows[i] = xs[i].numel() / std::max<int64_t>(cols, 1);
    parts[i] = colsum_parts(rows[i], cols);
    total += parts[i];
  }
  at::hip::HIPGuardMasqueradingAsCUDA guard(out.device());
  auto part = at::empty({total, cols}, xs[0].options().dtype(at::kFloat));
  auto s = cur_stream(out);
  int first = 0;
  bool uniform = true;
  for (size_t i = 1; i < xs.size(); ++i) uniform = uniform && rows[i] == rows[0];
  if (uniform && cols % 8 == 0) {
    // every segment's stage 1 in one launch per kColsumSegs inputs (grid.z = segment)
    for (size_t i0 = 0; i0 < xs.size(); i0 += kColsumSegs) {
      const int n = (int)std::min<size_t>(kColsumSegs, xs.size() - i0);
      ColsumSegs segs;
      for (int j = 0; j < n; ++j) segs.p[j] = xs[i0 + j].data_ptr();
      dispatch_fb(xs[0], "column_sum_segments", [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        MP_CHECK(column_sum_partial_multi<T>(segs, n, rows[0], (int)cols, ptr<float>(part) + (int64_t)first * cols,
                                             parts[0], s),
                 "column_sum_segments: multi-segment launch refused");
      });
      first += n * parts[0];
    }
    reduce_parts(ptr<float>(part), nullptr, total, (int)cols, out.data_ptr(), nullptr, out_f32, accumulate, s);
    return;
  }
  for (size_t i = 0; i < xs.size(); ++i) {
    dispatch_fb(xs[i], "column_sum_segments", [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      column_sum_partial<T>(cptr<T>(xs[i]), rows[i], (int)cols, ptr<float>(part) + (int64_t)first * cols, parts[i], s);
    });
    first += parts[i];
  }
  reduce_parts(ptr<float>(part), nullptr, total, (int)cols, out.data_ptr(), nullptr, out_f32, accumulate, s);
}

// The launches of a deferred weight gradient: `base` with up to GemmArgs::kMaxSegs micro-batches of as / bs as the
// K-segments of A / B each; the first one overwrites main_grad when !accumulate.  The bias gradient (optional, fp32
// [N]) is folded in through `fold_to` when the plan of every launch allows it (`fold_ok`); returns whether it was.
bool run_wgrad_segments(const char* name, const GemmArgs& base, const std::vector<Tensor>& as,
                        const std::vector<Tensor>& bs, bool accumulate, at::ScalarType dt, const Tensor& main_grad,
                        const std::optional<Tensor>& bias_grad, int64_t N, bool GemmPlan::*fold_ok,
                        float* GemmArgs::*fold_to) {
  const int total = (int)as.size();
  auto args_for = [&](int first) {
    const int n = std::min(GemmArgs::kMaxSegs, total - first);
    GemmArgs g = base;
    g.C = main_grad.data_ptr();
    g.K = base.seg_k * n;
    g.epi = (accumulate || first > 0) ? kEpiAccumF32 : kEpiStoreF32;
    for (int i = 0; i < n; ++i) {
      g.a_seg[i] = as[first + i].data_ptr();
      g.b_seg[i] = bs[first + i].data_ptr();
    }
    g.A = g.a_seg[0]; g.B = g.b_seg[0];
    return g;
  };
  bool fold = bias_grad && dt == at::kBFloat16;
  if (fold) {
    check_cuda(*bias_grad, "bias_grad");
    MP_CHECK(bias_grad->scalar_type() == at::kFloat && bias_grad->numel() == N && bias_grad->is_contiguous(), name,
             ": bias_grad must be a contiguous fp32 [N]");
    for (int first = 0; first < total && fold; first += GemmArgs::kMaxSegs) fold = gemm_plan(args_for(first)).*fold_ok;
  }
  for (int first = 0; first < total; first += GemmArgs::kMaxSegs) {
    GemmArgs g = args_for(first);
    if (fold) g.*fold_to = bias_grad->data_ptr<float>();
    Tensor ws = split_k_workspace(g, dt, main_grad);
    Tensor cws;
    if (g.colsum != nullptr && g.k_splits > 1) {  // per-split column sums, reduced after
      cws = at::empty({(int64_t)g.k_splits, N}, main_grad.options());
      g.colsum_ws = cws.data_ptr<float>();
    }
    gemm_run(dt, g, cur_stream(main_grad));
  }
  return fold;
}

// Deferred weight gradient over the micro-batches of a step:
//   main_grad[N, K] += sum_i dy_i^T . x_i
// as K-segmented GEMMs (up to GemmArgs::kMaxSegs micro-batches per launch),
// so the fp32 read-modify-write of main_grad happens once per launch instead
// of once per micro-batch and K is long enough to amortise the tile prologue.
// accumulate = false: the FIRST launch overwrites main_grad (its first write of
// the step after a lazy zero_grad), later launches accumulate.
// bias_grad (optional, fp32 [N]): the bias gradient colsum(dy) folded into the
// same GEMMs (GemmArgs::rowsum, accumulated); returns false (nothing added to
// bias_grad) when the shape cannot take the fold -- the caller then reduces it.
bool py_linear_wgrad_segments(std::vector<Tensor> dys, std::vector<Tensor> xs, Tensor main_grad, bool accumulate,
                              std::optional<Tensor> bias_grad) {
  MP_CHECK(!dys.empty() && dys.size() == xs.size(), "linear_wgrad_segments: need matching non-empty lists");
  check_cuda(main_grad, "main_grad");
  const int64_t T = dys[0].size(0), N = dys[0].size(1), K = xs[0].size(1);
  MP_CHECK(main_grad.scalar_type() == at::kFloat && main_grad.numel() == N * K, "linear_wgrad_segments: bad main_grad");
  const auto dt = dys[0].scalar_type();
  for (size_t i = 0; i < dys.size(); ++i) {
    check_gemm_2d(dys[i], "dy");
    check_gemm_2d(xs[i], "x");
    MP_CHECK(dys[i].scalar_type() == dt && xs[i].scalar_type() == dt, "linear_wgrad_segments: mixed dtypes");
    MP_CHECK(dys[i].size(0) == T && dys[i].size(1) == N && xs[i].size(0) == T && xs[i].size(1) == K,
             "linear_wgrad_segments: every micro-batch needs the same [T, N] / [T, K] shapes");
  }
  MP_CHECK(T % 64 == 0 && gemm_ok(dt, N, K, T), "linear_wgrad_segments: unsupported shape");
  const int64_t lda = row_stride(dys[0], "dy"), ldb = row_stride(xs[0], "x");
  for (size_t i = 1; i < dys.size(); ++i)
    MP_CHECK(row_stride(dys[i], "dy") == lda && row_stride(xs[i], "x") == ldb,
             "linear_wgrad_segments: every micro-batch needs the same row strides");
  at::hip::HIPGuardMasqueradingAsCUDA guard(main_grad.device());
  GemmArgs g;
  g.lda = lda; g.ldb = ldb; g.ldc = K; g.M = (int)N; g.N = (int)K; g.a_kc = false; g.b_kc = false; g.seg_k = (int)T;
  return run_wgrad_segments("linear_wgrad_segments", g, dys, xs, accumulate, dt, main_grad, bias_grad, N,
                            &GemmPlan::rowsum_ok, &GemmArgs::rowsum);
}

// The same deferred weight gradient from the transposed inputs x_i^T [K, T]
// (written by the forward GEMMs, linear_fwd(xt=...)):
//   main_grad[N, K] += sum_i (x_i^T . dy_i)^T
// computed as C^T[K, N] with A = x^T read K-contiguous and B = dy read [T, N]
// -- the dgrad layout, one transposing LDS read per operand instead of two
// (profiles/wgrad_layout_probe.txt) -- and stored transposed into main_grad.
// bias_grad: colsum(dy) folded into the same GEMMs (GemmArgs::colsum) when
// the shape allows (returns whether it was).
bool py_linear_wgrad_xt_segments(std::vector<Tensor> dys, std::vector<Tensor> xts, Tensor main_grad,
                                 bool accumulate, std::optional<Tensor> bias_grad) {
  MP_CHECK(!dys.empty() && dys.size() == xts.size(), "linear_wgrad_xt_segments: need matching non-empty lists");
  check_cuda(main_grad, "main_grad");
  const int64_t T = dys[0].size(0), N = dys[0].size(1), K = xts[0].size(0);
  MP_CHECK(main_grad.scalar_type() == at::kFloat && main_grad.numel() == N * K && main_grad.is_contiguous(),
           "linear_wgrad_xt_segments: bad main_grad");
  for (size_t i = 0; i < dys.size(); ++i) {
    check_gemm_2d(dys[i], "dy");
    check_gemm_2d(xts[i], "xt");
    MP_CHECK(dys[i].scalar_type() == at::kBFloat16 && xts[i].scalar_type() == at::kBFloat16,
             "linear_wgrad_xt_segments: bf16 operands only");
    MP_CHECK(dys[i].size(0) == T && dys[i].size(1) == N && xts[i].size(0) == K && xts[i].size(1) == T,
             "linear_wgrad_xt_segments: every micro-batch needs dy [T, N] and xt [K, T]");
  }
  MP_CHECK(T % 64 == 0 && K % 8 == 0 && gemm_supported(K, N, T), "linear_wgrad_xt_segments: unsupported shape");
  const int64_t lda = row_stride(xts[0], "xt"), ldb = row_stride(dys[0], "dy");
  for (size_t i = 1; i < dys.size(); ++i)
    MP_CHECK(row_stride(dys[i], "dy") == ldb && row_stride(xts[i], "xt") == lda,
             "linear_wgrad_xt_segments: every micro-batch needs the same row strides");
  at::hip::HIPGuardMasqueradingAsCUDA guard(main_grad.device());
  GemmArgs g;
  g.lda = lda; g.ldb = ldb; g.ldc = K; g.M = (int)K; g.N = (int)N; g.a_kc = true; g.b_kc = false; g.trans_c = true;
  g.seg_k = (int)T;
  return run_wgrad_segments("linear_wgrad_xt_segments", g, xts, dys, accumulate, at::kBFloat16, main_grad, bias_grad,
                            N, &GemmPlan::colsum_ok, &GemmArgs::colsum);
}

// Generic test entry: C[M,N] (fp32) = A . B with A given [M,K] (a_kc) or [K,M],
// B given [N,K] (b_kc) or [K,N].
Tensor py_gemm_f32(Tensor a, Tensor b, bool a_kc, bool b_kc) {
  check_gemm_2d(a, "a");
  check_gemm_2d(b, "b");
  check_same_dtype(a, b, "gemm");
  const auto dt = a.scalar_type();
  const int64_t M = a_kc ? a.size(0) : a.size(1);
  const int64_t K = a_kc ? a.size(1) : a.size(0);
  const int64_t N = b_kc ? b.size(0) : b.size(1);
  MP_CHECK((b_kc ? b.size(1) : b.size(0)) == K, "gemm: inner dims differ");
  MP_CHECK(gemm_ok(dt, M, N, K), "gemm: unsupported shape");
  at::hip::HIPGuardMasqueradingAsCUDA guard(a.device());
  auto c = at::empty({M, N}, a.options().dtype(at::kFloat));
  GemmArgs g;
  g.A = a.data_ptr(); g.B = b.data_ptr(); g.C = c.data_ptr();
  g.lda = row_stride(a, "a"); g.ldb = row_stride(b, "b"); g.ldc = N; g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.a_kc = a_kc; g.b_kc = b_kc; g.epi = kEpiStoreF32;
  gemm_run(dt, g, cur_stream(a));
  return c;
}

// gemm_plan of a bf16 GEMM given by scalars and flags (a flag: that operand or output is present): GemmPlan's
// fields in their declaration order.
py::tuple py_gemm_plan(int64_t M, int64_t N, int64_t K, bool a_kc, bool b_kc, int64_t epi, int64_t act, double p,
                       bool bias, bool aux, bool res, bool at, bool trans_c, bool rowsum, bool colsum, bool bits,
                       int64_t dact, int64_t seg_k, int64_t width, int64_t k_splits) {
  static float present[1];  // never read or written: the plan looks at which pointers are set
  const auto ptr_if = [](bool on) { return on ? present : nullptr; };
  GemmArgs g;
  g.M = (int)M; g.N = (int)N; g.K = (int)K; g.a_kc = a_kc; g.b_kc = b_kc; g.epi = (int)epi; g.act = (int)act;
  g.p = (float)p; g.trans_c = trans_c; g.seg_k = (int)seg_k; g.width = (int)width; g.k_splits = (int)k_splits;
  g.bias = ptr_if(bias); g.aux = ptr_if(aux); g.res = ptr_if(res); g.at = ptr_if(at); g.bits = ptr_if(bits);
  g.rowsum = ptr_if(rowsum); g.colsum = ptr_if(colsum); g.dact_in = ptr_if(dact != kActNone); g.dact = (int)dact;
  const GemmPlan pl = gemm_plan(g);
  return py::make_tuple(pl.big, pl.k_splits, pl.width, pl.extra, pl.x, pl.side, pl.kernel, pl.by_rounds, pl.along_n,
                        pl.per, pl.chunks, pl.rowsum_ok, pl.colsum_ok, pl.bits_ok);
}

// ------------------------------------------------------------------ attention
// q, k, v: [B, S, H, D] views (unit stride on D, identical strides), bf16.
// q, k, v: bf16 (attention.hip) or fp32 (attention_f32.hip).
void check_bshd(const Tensor& t, const char* name) {
  MP_CHECK(t.is_cuda() && (t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat), name,
           " must be a bf16 or fp32 GPU tensor");
  MP_CHECK(t.dim() == 4 && t.stride(3) == 1, name, " must be [B, S, H, D] with unit stride on D");
  const int64_t v = 16 / t.element_size();  // elements per 16 bytes
  MP_CHECK(t.stride(0) % v == 0 && t.stride(1) % v == 0 && t.stride(2) % v == 0 &&
               reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
           name, ": strides must keep 16-byte alignment");
}

bool attn_ok(at::ScalarType t, int S, int D) {
  return t == at::kFloat ? attention_f32_supported(S, D) : attention_supported(S, D);
}

// k and v may hold fewer heads than q (grouped-query attention: query head h reads K / V head
// h / group, group = H / Hkv) but share q's batch, token and head strides -- views of one packed
// projection.
void fill_qkv(AttnArgs& a, const Tensor& q, const Tensor& k, const Tensor& v) {
  check_bshd(q, "q");
  check_bshd(k, "k");
  check_bshd(v, "v");
  MP_CHECK(k.sizes() == v.sizes(), "attention: k, v shapes differ");
  MP_CHECK(q.size(0) == k.size(0) && q.size(1) == k.size(1) && q.size(3) == k.size(3) && k.size(2) > 0 &&
               q.size(2) % k.size(2) == 0,
           "attention: k, v must have q's batch, length and head dim and a head count dividing q's");
  MP_CHECK(q.strides() == k.strides() && q.strides() == v.strides(), "attention: q, k, v strides differ");
  MP_CHECK(q.scalar_type() == k.scalar_type() && q.scalar_type() == v.scalar_type(), "attention: q, k, v dtypes differ");
  a.q = q.data_ptr(); a.k = k.data_ptr(); a.v = v.data_ptr();
  a.B = (int)q.size(0); a.S = (int)q.size(1); a.H = (int)q.size(2); a.D = (int)q.size(3);
  a.group = (int)(q.size(2) / k.size(2));
  a.sb_qkv = q.stride(0); a.ld_qkv = q.stride(1); a.sh_qkv = q.stride(2);
  MP_CHECK(a.group == 1 || q.scalar_type() == at::kBFloat16,
           "attention: fewer K/V heads than query heads run on the bf16 kernels only (repeat the K/V heads for ",
           q.scalar_type(), ")");
  MP_CHECK(attn_group_ok(a.H, a.group), "attention: H=", a.H, " query heads over ", k.size(2), " K/V heads is too large");
  MP_CHECK(attn_ok(q.scalar_type(), a.S, a.D), "attention: unsupported S=", a.S, " D=", a.D, " for ",
           q.scalar_type(), " (bf16: S % 64 == 0, D in {64,128,256}; fp32: S % 32 == 0, D in {64,128})");
}

// bf16 D = 64, S >= 256 without a window, cap, document bounds or sinks run the long-sequence kernels
// (attention_long.hip); MIPIPE_ATTN_LONG=0 selects the previous kernels (A/B runs).
bool runs_long(const AttnArgs& a, const Tensor& q) {
  static const int on = [] {
    const char* e = getenv("MIPIPE_ATTN_LONG");
    return e == nullptr ? 1 : atoi(e);
  }();
  return on && a.window == 0 && a.softcap == 0.f && a.doc_start == nullptr && a.sinks == nullptr &&
         q.scalar_type() == at::kBFloat16 && attention_long_supported(a.S, a.D);
}

// Sliding-window attention (`window` keys per query, the query's own included; 0 = none): causal bf16 only,
// and always on attention.hip's generic kernels.  A window that covers the sequence is none.
int attn_window(const char* who, int64_t window, bool causal, const Tensor& q, int S) {
  MP_CHECK(window >= 0, who, ": window must be >= 0 (0 = none), got ", window);
  if (window == 0) return 0;
  MP_CHECK(causal, who, ": a sliding window needs causal attention");
  MP_CHECK(q.scalar_type() == at::kBFloat16, who, ": sliding-window attention runs on the bf16 kernels only, got ",
           q.scalar_type());
  return window >= S ? 0 : (int)window;
}

// Logit soft-capping (0 = none, else a finite cap > 0): bf16 only, and always on attention.hip's generic kernels.
float attn_softcap(const char* who, double softcap, const Tensor& q) {
  MP_CHECK(std::isfinite(softcap) && softcap >= 0.0, who, ": softcap must be a finite value >= 0 (0 = none), got ",
           softcap);
  if (softcap == 0.0) return 0.f;
  MP_CHECK(q.scalar_type() == at::kBFloat16, who, ": soft-capped attention runs on the bf16 kernels only, got ",
           q.scalar_type());
  const float c = (float)softcap;
  MP_CHECK(std::isfinite(c) && c > 0.f, who, ": softcap ", softcap, " is not a finite positive float");
  return c;
}

// Document-masked attention: `doc_bounds` int32 [B, 2, S] on q's device, contiguous (row 0: first token of each
// token's document, row 1: one past its last), causal bf16 only and always on attention.hip's generic kernels.
// Argument checks only: the values are the caller's contract (ops.check_doc_bounds), and the kernels clamp what
// they take from them.
void attn_docs(AttnArgs& a, const char* who, const std::optional<Tensor>& doc_bounds, bool causal, const Tensor& q) {
  if (!doc_bounds || !doc_bounds->defined()) return;
  const Tensor& d = *doc_bounds;
  MP_CHECK(causal, who, ": doc_bounds needs causal attention");
  MP_CHECK(q.scalar_type() == at::kBFloat16, who, ": document-masked attention runs on the bf16 kernels only, got ",
           q.scalar_type());
  MP_CHECK(d.scalar_type() == at::kInt, who, ": doc_bounds must be int32, got ", d.scalar_type());
  MP_CHECK(d.dim() == 3 && d.size(0) == a.B && d.size(1) == 2 && d.size(2) == a.S, who,
           ": doc_bounds must be [B, 2, S] = [", a.B, ", 2, ", a.S, "]");
  MP_CHECK(d.device() == q.device(), who, ": doc_bounds must be on q's device");
  MP_CHECK(d.is_contiguous(), who, ": doc_bounds must be contiguous");
  MP_CHECK(reinterpret_cast<uintptr_t>(d.data_ptr()) % 16 == 0, who, ": doc_bounds must be 16-byte aligned");
  a.doc_start = static_cast<const int32_t*>(d.data_ptr());
  a.doc_end = a.doc_start + a.S;
}

// Attention sinks: `sinks` fp32 [H] on q's device, contiguous, one logit per QUERY head; bf16 q/k/v only and
// always on attention.hip's generic kernels.  The values are free (-inf: no sink for that head).
void attn_sinks(AttnArgs& a, const char* who, const std::optional<Tensor>& sinks, const Tensor& q) {
  if (!sinks || !sinks->defined()) return;
  const Tensor& t = *sinks;
  MP_CHECK(q.scalar_type() == at::kBFloat16, who, ": attention with sinks runs on the bf16 kernels only, got ",
           q.scalar_type());
  MP_CHECK(t.scalar_type() == at::kFloat, who, ": sinks must be fp32, got ", t.scalar_type());
  MP_CHECK(t.dim() == 1 && t.size(0) == a.H, who, ": sinks must be [H] = [", a.H, "], one per query head");
  MP_CHECK(t.device() == q.device(), who, ": sinks must be on q's device");
  MP_CHECK(t.is_contiguous(), who, ": sinks must be contiguous");
  a.sinks = static_cast<const float*>(t.data_ptr());
}

// The options of both entry points (`who`, for the messages), checked and filled into `a` after fill_qkv.
void fill_options(AttnArgs& a, const char* who, const Tensor& q, bool causal, int64_t kv_len, int64_t window,
                  double softcap, const std::optional<Tensor>& doc_bounds, const std::optional<Tensor>& sinks) {
  attn_docs(a, who, doc_bounds, causal, q);
  attn_sinks(a, who, sinks, q);
  a.window = attn_window(who, window, causal, q, a.S);
  a.softcap = attn_softcap(who, softcap, q);
  MP_CHECK(kv_len == 0 || (q.scalar_type() == at::kFloat && kv_len > 0 && kv_len <= a.S), who,
           ": kv_len (a key-length bound) is for fp32, 0 < kv_len <= S");
  a.kv_len = (int)kv_len;
}

// Returns (o, lse, seed, offset, dropout keep bits): the bits tensor (int32
// [B*H, S/32, S]) is non-empty only for the long-sequence kernels with p > 0
// and must be handed back to attention_bwd.  A windowed call (0 < window < S) or a soft-capped one returns none.
// `words` (with the Philox draw it was made under): keep words an earlier forward of this same draw returned
// (a checkpoint's first forward, reused by its recompute) -- read instead of made, when the draw matches.
std::tuple<Tensor, Tensor, int64_t, int64_t, Tensor> py_attention_fwd(Tensor q, Tensor k, Tensor v, bool causal,
                                                                      double p, double scale, int64_t kv_len,
                                                                      std::optional<Tensor> words, int64_t words_seed,
                                                                      int64_t words_offset, int64_t window, double softcap,
                                                                      std::optional<Tensor> doc_bounds,
                                                                      std::optional<Tensor> sinks) {
  AttnArgs a;
  fill_qkv(a, q, k, v);
  fill_options(a, "attention", q, causal, kv_len, window, softcap, doc_bounds, sinks);
  MP_CHECK(p >= 0.0 && p < 1.0, "attention: bad dropout p");
  at::hip::HIPGuardMasqueradingAsCUDA guard(q.device());
  auto o = at::empty({a.B, a.S, a.H, a.D}, q.options());
  auto lse = at::empty({a.B, a.H, a.S}, q.options().dtype(at::kFloat));
  uint64_t seed = 0, offset = 0;
  if (p > 0.0) std::tie(seed, offset) = philox_draw(q.device(), 4);
  a.o = o.data_ptr(); a.sb_o = o.stride(0); a.ld_o = o.stride(1); a.sh_o = o.stride(2);
  a.lse = ptr<float>(lse);
  a.scale = (float)scale; a.p = (float)p; a.seed = seed; a.offset = offset; a.causal = causal;
  Tensor bits = at::empty({0}, q.options().dtype(at::kInt));
  if (q.scalar_type() == at::kFloat) {
    attention_f32_fwd(a, cur_stream(q));
  } else if (runs_long(a, q)) {
    bool reuse = false;
    if (p > 0.0) {
      const std::vector<int64_t> shape = {(int64_t)a.B * a.H, a.S / 32, a.S};
      reuse = words && words->defined() && words->sizes() == at::IntArrayRef(shape) &&
              words->scalar_type() == at::kInt && words->is_contiguous() && words->device() == q.device() &&
              (uint64_t)words_seed == seed && (uint64_t)words_offset == offset;
      bits = reuse ? *words : at::empty(shape, q.options().dtype(at::kInt));
      a.dmask = reinterpret_cast<uint32_t*>(bits.data_ptr());
    }
    if (reuse) attention_long_fwd_words(a, cur_stream(q));
    else attention_long_fwd(a, cur_stream(q));
  } else {
    attention_fwd(a, cur_stream(q));
  }
  return {o, lse, (int64_t)seed, (int64_t)offset, bits};
}

void py_attention_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, bool causal, double p,
                      double scale, int64_t seed, int64_t offset, Tensor dq, Tensor dk, Tensor dv,
                      std::optional<Tensor> bits, int64_t kv_len, int64_t window, double softcap,
                      std::optional<Tensor> doc_bounds, std::optional<Tensor> sinks, std::optional<Tensor> dsinks,
                      bool dsinks_accumulate) {
  AttnArgs a;
  fill_qkv(a, q, k, v);
  fill_options(a, "attention_bwd", q, causal, kv_len, window, softcap, doc_bounds, sinks);
  const bool want_dsinks = dsinks && dsinks->defined();
  if (want_dsinks) {
    MP_CHECK(a.sinks != nullptr, "attention_bwd: dsinks without sinks");
    MP_CHECK(dsinks->scalar_type() == at::kFloat && dsinks->dim() == 1 && dsinks->size(0) == a.H &&
                 dsinks->is_contiguous() && dsinks->device() == q.device(),
             "attention_bwd: dsinks must be a contiguous fp32 [H] = [", a.H, "] on q's device");
  }
  check_bshd(o, "o");
  check_bshd(dout, "dout");
  MP_CHECK(o.strides() == dout.strides() && o.sizes() == dout.sizes(), "attention_bwd: o/dout layout differs");
  MP_CHECK(o.scalar_type() == q.scalar_type() && dout.scalar_type() == q.scalar_type() &&
               dq.scalar_type() == q.scalar_type(), "attention_bwd: dtypes differ");
  MP_CHECK(dq.strides() == q.strides() && dk.strides() == q.strides() && dv.strides() == q.strides(),
           "attention_bwd: gradient buffers must share q's layout");
  MP_CHECK(dq.sizes() == q.sizes() && dk.sizes() == k.sizes() && dv.sizes() == k.sizes() &&
               dk.scalar_type() == q.scalar_type() && dv.scalar_type() == q.scalar_type(),
           "attention_bwd: gradient buffers must have q's / k's / v's shapes and dtype");
  MP_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == (int64_t)a.B * a.H * a.S, "attention_bwd: bad lse");
  at::hip::HIPGuardMasqueradingAsCUDA guard(q.device());
  auto delta = at::empty({a.B, a.H, a.S}, q.options().dtype(at::kFloat));
  a.o = o.data_ptr(); a.dout = dout.data_ptr();
  a.sb_o = o.stride(0); a.ld_o = o.stride(1); a.sh_o = o.stride(2);
  a.dq = dq.data_ptr(); a.dk = dk.data_ptr(); a.dv = dv.data_ptr();
  // Grouped-query attention: the dK / dV kernels keep one block per QUERY head and write its partial into a
  // scratch [B, S, 2, H, D]; gqa_reduce_dkv then sums each group into dk / dv, which must be the K and V head
  // slots of one packed contiguous dqkv [B, S, H + 2 Hkv, D] whose first H heads are dq.
  Tensor dkv;
  const int64_t Hkv = a.H / a.group, es = (int64_t)q.element_size();
  if (a.group > 1) {
    const int64_t ld = (a.H + 2 * Hkv) * (int64_t)a.D;
    const char* base = static_cast<const char*>(dq.data_ptr());
    MP_CHECK(dq.stride(2) == a.D && dq.stride(1) == ld && dq.stride(0) == ld * a.S &&
                 static_cast<const char*>(dk.data_ptr()) == base + (int64_t)a.H * a.D * es &&
                 static_cast<const char*>(dv.data_ptr()) == base + (a.H + Hkv) * a.D * es,
             "attention_bwd: with fewer K/V heads dq, dk, dv must be the head slices of one packed contiguous "
             "[B, S, H + 2 Hkv, D] gradient");
    dkv = at::empty({a.B, a.S, 2, a.H, a.D}, q.options());
    a.dk = dkv.data_ptr();
    a.dv = static_cast<char*>(dkv.data_ptr()) + (int64_t)a.H * a.D * es;
    a.sb_dkv = dkv.stride(0); a.ld_dkv = dkv.stride(1); a.sh_dkv = dkv.stride(3);
  }
  a.lse = ptr<float>(lse); a.delta = ptr<float>(delta);
  a.scale = (float)scale; a.p = (float)p; a.seed = (uint64_t)seed; a.offset = (uint64_t)offset; a.causal = causal;
  if (q.scalar_type() == at::kFloat) {
    attention_f32_bwd(a, cur_stream(q));
  } else if (runs_long(a, q)) {
    if (p > 0.0) {
      MP_CHECK(bits && bits->is_cuda() && bits->scalar_type() == at::kInt &&
                   bits->numel() == (int64_t)a.B * a.H * (a.S / 32) * a.S,
               "attention_bwd: the long-sequence kernels need the forward's dropout bits");
      a.dmask = reinterpret_cast<uint32_t*>(bits->data_ptr());
    }
    attention_long_bwd(a, cur_stream(q));
  } else {
    attention_bwd(a, cur_stream(q));
  }
  if (want_dsinks) {  // from the lse the forward stored and the delta the backward just wrote
    attention_dsink(a.lse, a.delta, a.sinks, ptr<float>(*dsinks), a.B, a.H, a.S, dsinks_accumulate, cur_stream(q));
  }
  if (a.group > 1) {
    gqa_reduce_dkv<bf16_t>(cptr<bf16_t>(dkv), static_cast<bf16_t*>(dq.data_ptr()), (int64_t)a.B * a.S, a.H, (int)Hkv,
                           a.D, cur_stream(q));
  }
}

// The sinks' gradient alone (attention_bwd runs it itself when given `dsinks`; this entry is for tools that time
// it): dsinks[h] (+)= -sum_{b,i} exp(sinks[h] - lse[b,h,i]) * delta[b,h,i].  fp32, contiguous, S % 4 == 0.
void py_attention_dsink(Tensor lse, Tensor delta, Tensor sinks, Tensor dsinks, bool accumulate) {
  for (const Tensor* t : {&lse, &delta, &sinks, &dsinks}) {
    MP_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->device() == lse.device(),
             "attention_dsink: lse, delta, sinks and dsinks must be contiguous fp32 tensors on one GPU");
  }
  MP_CHECK(lse.dim() == 3 && delta.sizes() == lse.sizes() && lse.size(2) % 4 == 0 && lse.size(1) > 0,
           "attention_dsink: lse and delta must be [B, H, S] with S % 4 == 0");
  MP_CHECK(sinks.dim() == 1 && sinks.size(0) == lse.size(1) && dsinks.sizes() == sinks.sizes(),
           "attention_dsink: sinks and dsinks must be [H] = [", lse.size(1), "]");
  at::hip::HIPGuardMasqueradingAsCUDA guard(lse.device());
  attention_dsink(cptr<float>(lse), cptr<float>(delta), cptr<float>(sinks), ptr<float>(dsinks), (int)lse.size(0),
                  (int)lse.size(1), (int)lse.size(2), accumulate, cur_stream(lse));
}

// ------------------------------------------------------------------ optimizer
Tensor py_sumsq(Tensor g) {
  check_cuda(g, "g");
  MP_CHECK(g.scalar_type() == at::kFloat, "sumsq: fp32 only");
  at::hip::HIPGuardMasqueradingAsCUDA guard(g.device());
  auto out = at::empty({1}, g.options());
  const int nparts = sumsq_parts(g.numel());
  auto part = at::empty({nparts}, g.options());
  sumsq(cptr<float>(g), g.numel(), ptr<float>(part), nparts, ptr<float>(out), cur_stream(g));
  return out;
}

void py_adam(Tensor master, std::optional<Tensor> model, Tensor grad, Tensor m, Tensor v, double lr, double b1,
             double b2, double eps, double wd, double bc1, double bc2, std::optional<Tensor> sumsq_t, double max_norm,
             bool adamw) {
  for (auto* t : {&master, &grad, &m, &v}) {
    check_cuda(*t, "adam buffer");
    MP_CHECK(t->scalar_type() == at::kFloat, "adam: master/grad/m/v must be fp32");
    MP_CHECK(t->numel() == master.numel(), "adam: size mismatch");
    MP_CHECK(t->is_contiguous() && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
             "adam: buffers must be contiguous and 16-byte aligned (vectorised kernel)");
  }
  if (model) {
    MP_CHECK(model->numel() == master.numel() && model->is_contiguous(), "adam: model size mismatch");
    MP_CHECK(reinterpret_cast<uintptr_t>(model->data_ptr()) % 16 == 0, "adam: model copy must be 16-byte aligned");
  }
  if (sumsq_t) MP_CHECK(sumsq_t->scalar_type() == at::kFloat && sumsq_t->numel() == 1, "adam: bad sumsq");
  at::hip::HIPGuardMasqueradingAsCUDA guard(master.device());
  AdamHyper h;
  h.lr = (float)lr; h.beta1 = (float)b1; h.beta2 = (float)b2; h.eps = (float)eps; h.weight_decay = (float)wd;
  h.bias_correction1 = (float)bc1; h.bias_correction2 = (float)bc2; h.max_norm = (float)max_norm; h.adamw = adamw;
  auto s = cur_stream(master);
  const float* sq = sumsq_t ? cptr<float>(*sumsq_t) : nullptr;
  if (!model) {
    adam_step<float>(ptr<float>(master), (float*)nullptr, cptr<float>(grad), ptr<float>(m), ptr<float>(v),
                     master.numel(), h, sq, s);
  } else if (model->scalar_type() == at::kBFloat16) {
    adam_step<bf16_t>(ptr<float>(master), ptr<bf16_t>(*model), cptr<float>(grad), ptr<float>(m), ptr<float>(v),
                      master.numel(), h, sq, s);
  } else {
    MP_CHECK(model->scalar_type() == at::kFloat, "adam: model copy must be bf16 or fp32");
    adam_step<float>(ptr<float>(master), ptr<float>(*model), cptr<float>(grad), ptr<float>(m), ptr<float>(v),
                     master.numel(), h, sq, s);
  }
}

}  // namespace
}  // namespace mipipe

// ------------------------------------------------------------------ ipc links
// Python face of mipipe::ipc::Link (runtime/ipc.h).  Host-blocking calls drop
// the GIL so watchdog threads keep running while a rank waits for its peer.
namespace {

namespace ipc = mipipe::ipc;

void ipc_check_tensor(const Tensor& t, const ipc::Link& L) {
  MP_CHECK(t.is_contiguous(), "ipc link: tensors must be contiguous");
  MP_CHECK(L.host_mode() ? !t.is_cuda() : t.is_cuda(), "ipc link: host links move CPU tensors, device links GPU tensors");
}

}  // namespace

// Defined in the build-generated source_digest.cpp (mipipe/build.py): the
// digest of the sources this binary was compiled from, checked at import by
// mipipe/_native_loader.py.
extern "C" const char* mipipe_source_digest();

PYBIND11_MODULE(_C, m) {
  m.def("source_digest", []() { return std::string(mipipe_source_digest()); });
  m.def("adam_set_variant", &mipipe::adam_set_variant);
  py::class_<ipc::Link>(m, "IpcLink")
      .def_static("create", &ipc::Link::create, py::arg("name"), py::arg("device"), py::arg("nslots"),
                  py::arg("slot_bytes"))
      .def_static("attach", &ipc::Link::attach, py::arg("name"), py::arg("device"), py::arg("engine") = 0,
                  py::arg("timeout") = 60.0, py::call_guard<py::gil_scoped_release>())
      .def("send",
           [](ipc::Link& L, Tensor src, int64_t producer, double timeout) {
             ipc_check_tensor(src, L);
             const void* p = src.data_ptr();
             const size_t n = src.nbytes();
             py::gil_scoped_release nogil;
             return L.send(p, n, reinterpret_cast<hipStream_t>(producer), timeout);
           },
           py::arg("src"), py::arg("producer_stream"), py::arg("timeout") = 300.0)
      .def("post", &ipc::Link::post)
      .def("wait",
           [](ipc::Link& L, uint64_t seq, Tensor dst, int64_t consumer, double timeout) {
             ipc_check_tensor(dst, L);
             void* p = dst.data_ptr();
             const size_t n = dst.nbytes();
             py::gil_scoped_release nogil;
             L.wait(seq, p, n, reinterpret_cast<hipStream_t>(consumer), timeout);
           },
           py::arg("seq"), py::arg("dst"), py::arg("consumer_stream"), py::arg("timeout") = 300.0)
      // Zero-copy receive (device links): the consumer stream waits for message
      // `seq` on the GPU and the returned tensor IS its slot (no copy), valid
      // until release(seq).  The tensor does not own the memory: the Link (and
      // its Python owner) must outlive it.
      .def("slot_tensor",
           [](ipc::Link& L, uint64_t seq, std::vector<int64_t> shape, py::object dtype, int64_t device) {
             MP_CHECK(!L.host_mode() && !L.is_sender(), "ipc slot_tensor: receiving device links only");
             const auto st = torch::python::detail::py_object_to_dtype(dtype);
             int64_t n = 1;
             for (auto d : shape) n *= d;
             MP_CHECK(n * (int64_t)c10::elementSize(st) <= L.slot_bytes(), "ipc slot_tensor: tensor larger than a slot");
             return at::from_blob(L.slot_ptr(seq), shape,
                                  at::TensorOptions().dtype(st).device(at::kCUDA, (c10::DeviceIndex)device));
           },
           py::arg("seq"), py::arg("shape"), py::arg("dtype"), py::arg("device"))
      .def("acquire",
           [](ipc::Link& L, uint64_t seq, int64_t consumer) { L.acquire(seq, reinterpret_cast<hipStream_t>(consumer)); },
           py::arg("seq"), py::arg("consumer_stream"))
      .def("release",
           [](ipc::Link& L, uint64_t seq, int64_t consumer) { L.release(seq, reinterpret_cast<hipStream_t>(consumer)); },
           py::arg("seq"), py::arg("consumer_stream"))
      // several messages at once: one counter write for the in-order prefix
      .def("release_many",
           [](ipc::Link& L, std::vector<uint64_t> seqs, int64_t consumer) {
             L.release(seqs, reinterpret_cast<hipStream_t>(consumer));
           },
           py::arg("seqs"), py::arg("consumer_stream"))
      .def("done", &ipc::Link::done)
      .def("abort", &ipc::Link::abort)
      .def("drain", &ipc::Link::drain, py::arg("timeout_s"), py::call_guard<py::gil_scoped_release>())
      .def("message_bytes", &ipc::Link::message_bytes)
      .def("unlink", &ipc::Link::unlink)
      .def("describe", &ipc::Link::describe)
      .def_property_readonly("copy_stream", [](const ipc::Link& L) { return reinterpret_cast<int64_t>(L.copy_stream()); })
      .def_property_readonly("inline_copy", &ipc::Link::inline_copy)
      .def_property_readonly("dma_engine", &ipc::Link::dma_engine)
      .def_property_readonly("nslots", &ipc::Link::nslots)
      .def_property_readonly("slot_bytes", &ipc::Link::slot_bytes)
      .def_property_readonly("host_mode", &ipc::Link::host_mode)
      .def_property_readonly("is_sender", &ipc::Link::is_sender);
  using namespace mipipe;
  m.doc() = "mipipe native runtime + CDNA4 HIP kernels (gfx950)";
  // runtime
  m.def("stream_pool_acquire", &py_stream_acquire, py::arg("device"), py::arg("priority") = -1);
  m.def("stream_wait", &py_stream_wait);
  m.def("peer_copy", &py_peer_copy, py::arg("dst"), py::arg("src"), py::arg("src_stream"), py::arg("dst_stream"),
        py::arg("src_device"), py::arg("dst_device"), py::arg("engine") = 0);
  m.def("enable_peer_access", [](std::vector<int> d) { rt::enable_peer_access(d); });
  m.def("can_access_peer", [](int d, int q) { return rt::can_access_peer(d, q); });
  m.def("copy_nocu",
        [](Tensor dst, Tensor src, int64_t stream) {
          MP_CHECK(dst.is_cuda() && src.is_cuda() && dst.nbytes() == src.nbytes(), "copy_nocu: equal device tensors");
          return rt::copy_nocu(dst.data_ptr(), src.data_ptr(), src.nbytes(), reinterpret_cast<hipStream_t>(stream));
        },
        py::arg("dst"), py::arg("src"), py::arg("stream"));
  m.def("hip_runtime_version", []() {
    int v = 0;
    (void)hipRuntimeGetVersion(&v);
    return v;
  });
  m.def("range_push", [](const std::string& s) { rt::range_push(s); });
  m.def("range_pop", []() { rt::range_pop(); });
  m.def("mark", [](const std::string& s) { rt::mark(s); });
  m.def("gpu_sleep", &py_gpu_sleep);
  m.def("philox_draw", [](int64_t device, int64_t inc) {
    auto r = philox_draw(at::Device(at::kCUDA, (c10::DeviceIndex)device), (uint64_t)inc);
    return std::make_pair((int64_t)r.first, (int64_t)r.second);
  });
  // kernels
  m.def("layernorm_fwd", &py_layernorm_fwd);
  m.def("layernorm_bwd", &py_layernorm_bwd, py::arg("dy"), py::arg("z"), py::arg("mean"), py::arg("rstd"),
        py::arg("gamma"), py::arg("p"), py::arg("seed"), py::arg("offset"), py::arg("acc_gamma") = py::none(),
        py::arg("acc_beta") = py::none(), py::arg("addend") = py::none());
  m.def("rmsnorm_fwd", &py_rmsnorm_fwd, py::arg("x"), py::arg("res"), py::arg("gamma"), py::arg("eps"), py::arg("p"),
        py::arg("save_z"));
  m.def("rmsnorm_bwd", &py_rmsnorm_bwd, py::arg("dy"), py::arg("z"), py::arg("rstd"), py::arg("gamma"), py::arg("p"),
        py::arg("seed"), py::arg("offset"), py::arg("acc_gamma") = py::none(), py::arg("addend") = py::none());
  m.def("swiglu_fwd", &py_swiglu_fwd);
  m.def("swiglu_bwd", &py_swiglu_bwd);
  m.def("geglu_fwd", &py_geglu_fwd);
  m.def("geglu_bwd", &py_geglu_bwd);
  m.def("rmsnorm_residual_fwd", &py_rmsnorm_residual_fwd, py::arg("x"), py::arg("res"), py::arg("gamma"),
        py::arg("eps"), py::arg("save"));
  m.def("rope_packed", &py_rope_packed, py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("out") = py::none(),
        py::arg("pos0") = 0, py::arg("inverse") = false);
  m.def("rope_heads", &py_rope_heads, py::arg("x"), py::arg("cos"), py::arg("sin"), py::arg("out") = py::none(),
        py::arg("n_rot"), py::arg("pos0") = 0, py::arg("inverse") = false,
        "x [B, S, heads, D]: the first n_rot heads of every token rotated, the rest passed through");
  m.def("gqa_reduce_dkv", &py_gqa_reduce_dkv, py::arg("dkv"), py::arg("dqkv"), py::arg("H"), py::arg("Hkv"),
        "dkv [B, S, 2, H, D] per-query-head dK / dV partials -> group sums in the K / V heads of dqkv "
        "[B, S, H + 2 Hkv, D]");
  m.def("qk_norm_rope_supported", [](int64_t D) { return D > 0 && D <= 256 && qknorm_supported((int)D); });
  m.def("qk_norm_rope_fwd", &py_qk_norm_rope_fwd, py::arg("x"), py::arg("wq"), py::arg("wk"), py::arg("eps"),
        py::arg("cos") = py::none(), py::arg("sin") = py::none(), py::arg("out") = py::none(), py::arg("n_q"),
        py::arg("n_k"), py::arg("pos0") = 0, py::arg("save_rstd") = true,
        "x [B, S, heads, D]: per-head RMSNorm of the first n_q (wq) and next n_k (wk) heads, then rotated (no "
        "tables: the norm alone); the rest passed through.  Returns (y, rstd or None)");
  m.def("qk_norm_rope_bwd", &py_qk_norm_rope_bwd, py::arg("dout"), py::arg("x"), py::arg("rstd"), py::arg("wq"),
        py::arg("wk"), py::arg("cos") = py::none(), py::arg("sin") = py::none(), py::arg("n_q"), py::arg("n_k"),
        py::arg("pos0") = 0, py::arg("acc_q") = py::none(), py::arg("acc_k") = py::none(),
        "(dx, dwq, dwk); a weight gradient with an fp32 accumulation target is added there and returned as None");
  m.def("moe_route_supported",
        [](int64_t n_experts, int64_t k) { return n_experts <= 256 && k <= 8 && moe_route_supported((int)n_experts, (int)k); });
  m.def("moe_route_fwd", &py_moe_route_fwd, py::arg("logits"), py::arg("k"),
        "logits [T, Ne] -> (idx int32 [T, k], gate fp32 [T, k], probs_sum fp32 [Ne])");
  m.def("moe_route_bwd", &py_moe_route_bwd, py::arg("logits"), py::arg("idx"), py::arg("gate"), py::arg("dgate"),
        py::arg("dprobs") = py::none());
  m.def("moe_assign", &py_moe_assign, py::arg("idx"), py::arg("n_experts"), py::arg("capacity"),
        "idx int32 [T, k] -> (slot int32 [T, k], src int32 [Ne * C], counts int32 [Ne])");
  m.def("moe_assign_sorted", &py_moe_assign_sorted, py::arg("idx"), py::arg("n_experts"), py::arg("rows"),
        "idx int32 [T, k] -> (slot [T, k], src [rows], counts [Ne], offsets [Ne + 1], tile_expert [rows / 128])");
  m.def("grouped_gemm_supported", &grouped_gemm_supported, py::arg("rows"), py::arg("n_out"), py::arg("reduction"));
  m.def("grouped_gemm_rows", &py_grouped_gemm_rows, py::arg("a"), py::arg("wptrs"), py::arg("tile_expert"),
        py::arg("n_out"), py::arg("w_kc"));
  m.def("grouped_gemm_wgrad", &py_grouped_gemm_wgrad, py::arg("dy"), py::arg("x"), py::arg("offsets"),
        py::arg("optrs") = py::none(), py::arg("accumulate") = false);
  m.def("moe_gather_slots", &py_moe_gather_slots, py::arg("x"), py::arg("src"), py::arg("k"));
  m.def("moe_gather_tokens", &py_moe_gather_tokens, py::arg("ye"), py::arg("slot"), py::arg("w") = py::none(),
        py::arg("res") = py::none());
  m.def("moe_combine_bwd", &py_moe_combine_bwd, py::arg("dy"), py::arg("ye"), py::arg("gate"), py::arg("src"));
  m.def("bias_act_fwd", &py_bias_act_fwd);
  m.def("softcap_fwd", &py_softcap_fwd, py::arg("x"), py::arg("cap"), py::arg("out") = py::none());
  m.def("softcap_bwd", &py_softcap_bwd, py::arg("dy"), py::arg("y"), py::arg("cap"), py::arg("out") = py::none());
  m.def("bias_act_bwd", &py_bias_act_bwd, py::arg("dy"), py::arg("saved"), py::arg("bias"), py::arg("act"),
        py::arg("p"), py::arg("seed"), py::arg("offset"), py::arg("need_dbias"), py::arg("dbias_acc") = py::none());
  m.def("column_sum", &py_column_sum, py::arg("x"), py::arg("out") = py::none(), py::arg("accumulate") = false);
  m.def("cross_entropy_fwd", &py_ce_fwd, py::arg("logits"), py::arg("target"), py::arg("ignore_index"),
        py::arg("t_offset") = 0);
  m.def("cross_entropy_bwd", &py_ce_bwd, py::arg("logits"), py::arg("target"), py::arg("lse"), py::arg("scale"),
        py::arg("ignore_index"), py::arg("row_scale") = py::none(), py::arg("out") = py::none(),
        py::arg("zero_pad") = false, py::arg("t_offset") = 0, py::arg("stat_out") = py::none());
  m.def("cross_entropy_mean_fwd", &py_ce_mean_fwd, py::arg("logits"), py::arg("target"), py::arg("ignore_index"));
  m.def("vsplit_head_fwd", &py_vsplit_head_fwd);
  m.def("vsplit_tail_fwd", &py_vsplit_tail_fwd);
  m.def("embedding_fwd", &py_embed_fwd);
  m.def("embedding_bwd", &py_embed_bwd, py::arg("tokens"), py::arg("dout"), py::arg("dweight"), py::arg("scale"),
        py::arg("p"), py::arg("seed"), py::arg("offset"), py::arg("dpe") = py::none());
  m.def("attention_supported", [](int64_t S, int64_t D) { return attention_supported((int)S, (int)D); });
  m.def("attention_f32_supported", [](int64_t S, int64_t D) { return attention_f32_supported((int)S, (int)D); });
  m.def("attention_fwd", &py_attention_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("causal"), py::arg("p"),
        py::arg("scale"), py::arg("kv_len") = 0, py::arg("words") = py::none(), py::arg("words_seed") = 0,
        py::arg("words_offset") = 0, py::arg("window") = 0, py::arg("softcap") = 0.0,
        py::arg("doc_bounds") = py::none(), py::arg("sinks") = py::none());
  m.def("attention_bwd", &py_attention_bwd, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("causal"), py::arg("p"), py::arg("scale"), py::arg("seed"), py::arg("offset"),
        py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("bits") = py::none(), py::arg("kv_len") = 0,
        py::arg("window") = 0, py::arg("softcap") = 0.0, py::arg("doc_bounds") = py::none(),
        py::arg("sinks") = py::none(), py::arg("dsinks") = py::none(), py::arg("dsinks_accumulate") = false);
  m.def("attention_dsink", &py_attention_dsink, py::arg("lse"), py::arg("delta"), py::arg("sinks"), py::arg("dsinks"),
        py::arg("accumulate") = false);
  m.def("attention_long_supported", [](int64_t S, int64_t D) { return attention_long_supported((int)S, (int)D); });
  m.def("attention_long_set_fused_rng", &attention_long_set_fused_rng,
        "long-sequence attention: make the dropout keep words inside the forward kernel (true, default) or in a "
        "kernel of their own before it (false)");
  m.def("gemm_supported", &gemm_supported);
  m.def("gemm_f32_supported", &gemm_f32_supported);
  m.def("attention_set_fused_bwd", &attention_set_fused_bwd);
  m.def("gemm_set_rounds", &gemm_set_rounds,
        "multi-round GEMM grids whose last round is at most half full: 0 one launch, 1 (default) one launch per round "
        "of tiles when K >= 4096, 2 one launch per round at any K");
  m.def("gemm_set_splitk", &gemm_set_splitk, "split-K factor of under-filled long-K GEMMs: 0 off, 1 auto (default), n >= 2 forced");
  m.def("gemm_set_width", &gemm_set_width, "256-row GEMM block width: 0 auto (grid-quantisation rule), 128, 256");
  m.def("linear_fwd", &py_linear_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("act"), py::arg("p"),
        py::arg("save_preact"), py::arg("res") = py::none(), py::arg("xt") = py::none(),
        py::arg("aux_grad") = false, py::arg("bits") = py::none());
  m.def("gemm_plan", &py_gemm_plan, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("a_kc") = true,
        py::arg("b_kc") = true, py::arg("epi") = 0, py::arg("act") = 0, py::arg("p") = 0.0, py::arg("bias") = false,
        py::arg("aux") = false, py::arg("res") = false, py::arg("at") = false, py::arg("trans_c") = false,
        py::arg("rowsum") = false, py::arg("colsum") = false, py::arg("bits") = false, py::arg("dact") = 0,
        py::arg("seg_k") = 0, py::arg("width") = 0, py::arg("k_splits") = 1,
        "how the bf16 GEMM launches these arguments: (big, k_splits, width, extra, x, side, kernel, by_rounds, along_n, "
        "per, chunks, rowsum_ok, colsum_ok, bits_ok), see GemmPlan");
  m.def("linear_bits_ok",
        [](int64_t M, int64_t N, int64_t K, int64_t act, double p) {
          GemmArgs g;
          g.M = (int)M; g.N = (int)N; g.K = (int)K; g.act = (int)act; g.p = (float)p;
          g.a_kc = true; g.b_kc = true; g.epi = kEpiStoreAct;
          return gemm_supported(M, N, K) && gemm_plan(g).bits_ok;
        },
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("act"), py::arg("p"),
        "whether linear_fwd can also write the ReLU output's nonzero mask as bits (kActReluBits)");
  m.def("gemm_emit_ok", &gemm_emit_ok, py::arg("act"), py::arg("p"), py::arg("aux"),
        "whether linear_fwd can also write x^T for this activation / dropout / pre-activation output");
  m.def("linear_wgrad_xt_segments", &py_linear_wgrad_xt_segments, py::arg("dys"), py::arg("xts"),
        py::arg("main_grad"), py::arg("accumulate") = true, py::arg("bias_grad") = py::none());
  m.def("linear_dgrad", &py_linear_dgrad, py::arg("dy"), py::arg("w"), py::arg("res") = py::none(),
        py::arg("out") = py::none(), py::arg("act") = 0, py::arg("saved") = py::none(), py::arg("p") = 0.0,
        py::arg("seed") = 0, py::arg("offset") = 0);
  m.def("linear_wgrad", &py_linear_wgrad, py::arg("dy"), py::arg("x"), py::arg("main_grad"),
        py::arg("accumulate") = true);
  m.def("linear_wgrad_segments", &py_linear_wgrad_segments, py::arg("dys"), py::arg("xs"), py::arg("main_grad"),
        py::arg("accumulate") = true, py::arg("bias_grad") = py::none());
  m.def("column_sum_segments", &py_column_sum_segments);
  m.def("transpose_b16", &py_transpose_b16);
  m.def("gemm_f32", &py_gemm_f32);
  m.def("sumsq", &py_sumsq);
  m.def("adam_step", &py_adam);
}
