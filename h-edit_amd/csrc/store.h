// The parameter store every network handle derives from, and the C-ABI lifecycle every handle family shares.
//
// A network registers its parameters by their state_dict names at create time (vec / mat / f32conv / lin / conv3 / twin /
// add_slot); hedit_<fam>_load then packs one checkpoint tensor into every destination its slot names.  The store owns the device
// allocations.  The code is in store.hip, compiled once; everything here has hidden visibility (it is not part of the C ABI).
//
// HEDIT_LIFECYCLE(fam, type, what, pre_destroy) at file scope generates hedit_<fam>_destroy / _num_params / _param_name /
// _param_shape / _load / _missing of include/hedit.h, and the three checks a family's own entries use: handle_created (the
// allocation-failure epilogue of create), handle_loaded ("<what> has N unloaded parameters") and handle_finalized ("call
// hedit_<fam>_finalize after loading the parameters").  pre_destroy(h) runs first in destroy (an outstanding tape, profiler events).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/hedit.h"
#include "common.h"

#pragma GCC visibility push(hidden)

// how a checkpoint tensor (fp32, torch layout, on the device) is written into one destination
enum class Pack {
  F32,            // fp32 copy
  Linear,         // [O][I] -> bf16, times scale
  Conv3,          // conv3x3 OIHW -> bf16 [O][9][I]
  GegluRows,      // FF1 weight [2N][I] -> bf16 with the GEGLU (value16 | gate16) row interleave
  GegluBias,      // FF1 bias in the same row order, fp32
  FfnLayer,       // layer `which` of the block-tail weight stream of ffn.hip
  FfnBias,        // the FF1 bias in that kernel's packed order
  ChainLayer,     // layer `which` of a projection-chain weight stream of `lay` layers (linchain.hip), times scale
  LinearT,        // [O][I] -> bf16 [I][O], times scale, rows `ld` apart (0 = dense): the input-gradient twin of a linear
  Conv3Dgrad,     // conv3x3 -> bf16 [I][9][O], taps flipped: the input-gradient twin of a stride-1 convolution
  Conv3S2Dgrad,   // the same with the taps in place (stride-2 dgrad)
  FlipOIHW,       // OIHW -> fp32 IOHW, taps flipped
};

struct PackDst {
  Pack kind;
  void* dst;
  float scale = 1.f;
  long ld = 0;
  int which = 0, lay = 0;
};

struct ParamSlot {
  std::string name;
  size_t numel;
  int O, I;          // what the packers take (0 where the kind needs neither)
  int ndim;
  int dims[4];       // the torch shape
  bool loaded;
  PackDst to;
  std::vector<PackDst> more;   // further destinations of the same tensor: input-gradient twins, unfused copies
};

// parameters of one network, owned device copies; the public handles derive from this
struct ParamStore {
  bool alloc_failed = false;
  bool finalized = false;      // families with a finalize step: set by it, cleared by every load
  std::vector<void*> owned;
  std::vector<ParamSlot> slots;
  std::map<std::string, int> index;
};

void* store_alloc(ParamStore* h, size_t bytes);      // nullptr + alloc_failed on failure
void store_free(ParamStore* h);
template <class T>
T* dalloc(ParamStore* h, size_t n) { return reinterpret_cast<T*>(store_alloc(h, n * sizeof(T))); }

ParamSlot& add_slot(ParamStore* h, const std::string& name, Pack kind, void* dst, size_t numel, int O, int I, int ndim,
                    int d0, int d1, int d2, int d3);
// dst: a place inside a larger allocation of the caller's (stacked matrices); nullptr = allocated here
float* vec(ParamStore* h, const std::string& name, int n, float* dst = nullptr);
float* mat(ParamStore* h, const std::string& name, int O, int I);             // a [O][I] matrix kept fp32 (packed by the executor's finalize)
float* f32conv(ParamStore* h, const std::string& name, int O, int I, int k);  // kept fp32, torch layout
bf16_t* lin(ParamStore* h, const std::string& name, int O, int I, bool conv1x1 = false, bf16_t* dst = nullptr, float scale = 1.f);
bf16_t* conv3(ParamStore* h, const std::string& name, int O, int I);          // at least 4 rows, zero beyond O (N = 4 GEMM route)
void* add_dst(ParamStore* h, Pack kind, void* dst, size_t bytes, float scale, long ld);
// one more destination for the slot just added (its O, I); dst as above
template <class T>
T* twin(ParamStore* h, Pack kind, size_t n, T* dst = nullptr, float scale = 1.f, long ld = 0) {
  return reinterpret_cast<T*>(add_dst(h, kind, dst, n * sizeof(T), scale, ld));
}

// what: the network's display name in "unknown <what> parameter" (empty: "unknown parameter")
int store_load(ParamStore* h, const char* what, const char* name, const float* w, size_t numel, hipStream_t st);
int store_missing(const ParamStore* h);
int store_num_params(const ParamStore* h);
const char* store_param_name(const ParamStore* h, int i);
int store_param_shape(const ParamStore* h, int i, int* ndim, int* dims4);
// 1: kept as an unscaled bf16 copy (matrices, convolutions), so handing it over rounded to bf16 loses nothing; 0: kept in fp32
// or scaled while packed
int store_param_bf16_exact(const ParamStore* h, int i);
int store_require_created(ParamStore* h, const char* fam);         // HEDIT_ERR_HIP if an allocation failed
int store_require_loaded(const ParamStore* h, const char* what);   // HEDIT_ERR_STATE "<what> has N unloaded parameters"
int store_require_finalized(const ParamStore* h, const char* fam);

inline void no_pre_destroy(ParamStore*) {}
// a handle type `struct HEDIT_HANDLE hedit_<fam> : ParamStore`: its implicit members are no more exported than the store's
#define HEDIT_HANDLE __attribute__((visibility("hidden")))

#pragma GCC visibility pop

#define HEDIT_LIFECYCLE(fam, T, what, pre_destroy)                                                                        \
  extern "C" {                                                                                                            \
  void hedit_##fam##_destroy(T* h) try {                                                                                  \
    if (!h) return;                                                                                                       \
    pre_destroy(h);                                                                                                       \
    store_free(h);                                                                                                        \
    delete h;                                                                                                             \
  } catch (...) { (void)hedit_abi_catch(); }                                                                              \
  int hedit_##fam##_num_params(const T* h) { return store_num_params(h); }                                                \
  const char* hedit_##fam##_param_name(const T* h, int i) try {                                                           \
    return store_param_name(h, i);                                                                                        \
  } catch (...) { (void)hedit_abi_catch(); return nullptr; }                                                              \
  int hedit_##fam##_param_shape(const T* h, int i, int* ndim, int* dims4) try {                                           \
    return store_param_shape(h, i, ndim, dims4);                                                                          \
  } catch (...) { return hedit_abi_catch(); }                                                                             \
  int hedit_##fam##_load(T* h, const char* name, const float* w, size_t numel, void* stream) try {                        \
    ARG_CHECK(h && name && w, "null");                                                                                    \
    return store_load(h, what, name, w, numel, reinterpret_cast<hipStream_t>(stream));                                    \
  } catch (...) { return hedit_abi_catch(); }                                                                             \
  int hedit_##fam##_missing(const T* h) try { return h ? store_missing(h) : -1; } catch (...) { return hedit_abi_catch(); } \
  }                                                                                                                       \
  /* the epilogue of create: publish the handle, or destroy it if an allocation failed */                                 \
  [[maybe_unused]] static int handle_created(T* h, T** out) {                                                             \
    const int rc = store_require_created(h, #fam);                                                                        \
    if (rc != HEDIT_OK) hedit_##fam##_destroy(h);                                                                         \
    else *out = h;                                                                                                        \
    return rc;                                                                                                            \
  }                                                                                                                       \
  [[maybe_unused]] static int handle_loaded(const T* h) { return store_require_loaded(h, what); }                        \
  [[maybe_unused]] static int handle_finalized(const T* h) { return store_require_finalized(h, #fam); }
