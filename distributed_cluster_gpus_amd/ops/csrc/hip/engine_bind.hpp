// One checked binder from named torch tensors to EngineDesc pointer fields:
//
//   Binder bind(tensors);
//   bind(S_.now, "now", R);          // double*   <- float64, >= R elements
//   bind(S_.s_rec, "s_rec", R * TS); // SRec*     <- float64 rows of 8
//
// The element type comes from the field, the tensor dtype from ElemOf below.
// A bound tensor is present, of that dtype, contiguous, on the same device as
// every other bound tensor and at least `need` field elements long; anything
// else throws std::invalid_argument naming the field, what was required and
// what was found.  The binds, in order, are the engine's contract().
#pragma once
#include <torch/extension.h>

#include <string>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "engine_desc.hpp"

namespace dcg {

// field element type -> tensor dtype.  The same-width aliases (a field type
// torch has no name for, or a packed record over float64 rows) are stated
// here and nowhere else.
template <class T> struct ElemOf;
#define DCG_ELEM(T, ST) \
  template <> struct ElemOf<T> { static constexpr auto dtype = torch::ST; }
DCG_ELEM(double, kFloat64);
DCG_ELEM(float, kFloat32);
DCG_ELEM(int, kInt32);
DCG_ELEM(short, kInt16);
DCG_ELEM(char, kInt8);
DCG_ELEM(unsigned char, kUInt8);
DCG_ELEM(long long, kInt64);
DCG_ELEM(uint64_t, kInt64);
DCG_ELEM(SRec, kFloat64);
DCG_ELEM(XRec, kFloat64);
DCG_ELEM(ARec, kFloat64);
#undef DCG_ELEM

class Binder {
 public:
  // (field, dtype, required numel in tensor elements; -1 = this configuration
  // never dereferences the field, so it is neither bound nor checked)
  using Row = std::tuple<std::string, std::string, int64_t>;

  explicit Binder(const std::unordered_map<std::string, torch::Tensor>& t)
      : t_(t) {}

  template <class P>
  void operator()(P*& field, const char* name, int64_t need) {
    using E = std::remove_const_t<P>;
    const auto dtype = ElemOf<E>::dtype;
    const int64_t item = (int64_t)c10::elementSize(dtype);
    const int64_t per = (int64_t)sizeof(E) / item;  // tensor elements per E
    const int64_t numel = need * per;
    const std::string want = std::string(c10::toString(dtype)) + "[>=" +
                             std::to_string(numel) + "] contiguous" +
                             (per > 1 ? ", rows of " + std::to_string(per) : "");
    auto it = t_.find(name);
    if (it == t_.end()) fail(name, want, "no such tensor");
    const torch::Tensor& x = it->second;
    if (need < 0 || x.scalar_type() != dtype || !x.is_contiguous() ||
        x.numel() < numel || (per > 1 && (x.dim() < 1 || x.size(-1) != per)) ||
        (bound_ && x.device() != device_))
      fail(name, want + (bound_ ? " on " + device_.str() : ""), describe(x));
    if (!bound_) { device_ = x.device(); bound_ = true; }
    field = static_cast<P*>(x.data_ptr());
    rows_.emplace_back(name, c10::toString(dtype), numel);
  }

  // a field this configuration's kernel never dereferences
  void unused(const char* name) { rows_.emplace_back(name, "", -1); }

  const std::vector<Row>& rows() const { return rows_; }
  bool on_gpu() const { return bound_ && device_.is_cuda(); }
  std::string device_str() const { return bound_ ? device_.str() : "none"; }

 private:
  static std::string describe(const torch::Tensor& x) {
    std::string s = std::string(c10::toString(x.scalar_type())) + "[";
    for (int64_t d = 0; d < x.dim(); ++d)
      s += (d ? ", " : "") + std::to_string(x.size(d));
    return s + "] (" + std::to_string(x.numel()) + " elements) " +
           (x.is_contiguous() ? "contiguous" : "NON-contiguous") + " on " +
           x.device().str();
  }
  [[noreturn]] static void fail(const char* name, const std::string& want,
                                const std::string& found) {
    throw std::invalid_argument(std::string("engine tensor '") + name +
                                "': required " + want + ", found " + found);
  }

  const std::unordered_map<std::string, torch::Tensor>& t_;
  std::vector<Row> rows_;
  c10::Device device_{c10::kCPU};
  bool bound_ = false;
};

}  // namespace dcg
