// The parameter store behind every network handle (store.h): registration, the one loader, the parameter table.
#include "store.h"

#include "kernels.h"

#define TRY(expr)                        \
  do {                                   \
    int _rc = (expr);                    \
    if (_rc != HEDIT_OK) return _rc;     \
  } while (0)

void* store_alloc(ParamStore* h, size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes > 0 ? bytes : 16) != hipSuccess) {
    h->alloc_failed = true;
    return nullptr;
  }
  h->owned.push_back(p);
  return p;
}

void store_free(ParamStore* h) {
  for (void* p : h->owned) if (p) (void)hipFree(p);
  h->owned.clear();
}

ParamSlot& add_slot(ParamStore* h, const std::string& name, Pack kind, void* dst, size_t numel, int O, int I, int ndim,
                    int d0, int d1, int d2, int d3) {
  h->index[name] = (int)h->slots.size();
  h->slots.push_back(ParamSlot{name, numel, O, I, ndim, {d0, d1, d2, d3}, false, PackDst{kind, dst}, {}});
  return h->slots.back();
}

float* vec(ParamStore* h, const std::string& name, int n, float* dst) {
  if (!dst) dst = dalloc<float>(h, n);
  add_slot(h, name, Pack::F32, dst, n, 0, 0, 1, n, 1, 1, 1);
  return dst;
}
float* mat(ParamStore* h, const std::string& name, int O, int I) {
  float* d = dalloc<float>(h, (size_t)O * I);
  add_slot(h, name, Pack::F32, d, (size_t)O * I, O, I, 2, O, I, 1, 1);
  return d;
}
float* f32conv(ParamStore* h, const std::string& name, int O, int I, int k) {
  float* d = dalloc<float>(h, (size_t)O * I * k * k);
  add_slot(h, name, Pack::F32, d, (size_t)O * I * k * k, O, I, 4, O, I, k, k);
  return d;
}
bf16_t* lin(ParamStore* h, const std::string& name, int O, int I, bool conv1x1, bf16_t* dst, float scale) {
  if (!dst) dst = dalloc<bf16_t>(h, (size_t)O * I);
  add_slot(h, name, Pack::Linear, dst, (size_t)O * I, O, I, conv1x1 ? 4 : 2, O, I, 1, 1).to.scale = scale;
  return dst;
}
bf16_t* conv3(ParamStore* h, const std::string& name, int O, int I) {
  // at least 4 rows (zero beyond O): a conv with <= 4 output channels can then run as an N = 4 GEMM
  const int rows = O < 4 ? 4 : O;
  bf16_t* d = dalloc<bf16_t>(h, (size_t)rows * I * 9);
  if (d && rows != O && hipMemset(d, 0, (size_t)rows * I * 9 * sizeof(bf16_t)) != hipSuccess) h->alloc_failed = true;
  add_slot(h, name, Pack::Conv3, d, (size_t)O * I * 9, O, I, 4, O, I, 3, 3);
  return d;
}
void* add_dst(ParamStore* h, Pack kind, void* dst, size_t bytes, float scale, long ld) {
  if (!dst) dst = store_alloc(h, bytes);
  h->slots.back().more.push_back(PackDst{kind, dst, scale, ld});
  return dst;
}

static int pack(const ParamSlot& s, const PackDst& d, const float* w, hipStream_t st) {
  bf16_t* d16 = reinterpret_cast<bf16_t*>(d.dst);
  float* d32 = reinterpret_cast<float*>(d.dst);
  switch (d.kind) {
    case Pack::F32: HIP_TRY(hipMemcpyAsync(d.dst, w, s.numel * sizeof(float), hipMemcpyDeviceToDevice, st)); return HEDIT_OK;
    case Pack::Linear: return pack_linear_launch(w, d16, (long)s.numel, d.scale, st);
    case Pack::Conv3: return pack_conv3x3_launch(w, d16, s.O, s.I, st);
    case Pack::GegluRows: return pack_geglu_rows_launch(w, d16, nullptr, s.O, s.I, st);
    case Pack::GegluBias: return pack_geglu_rows_launch(w, nullptr, d32, (int)s.numel, 1, st);
    case Pack::FfnLayer: return ffn_pack_launch(w, d.which, 1, 1, d16, st);
    case Pack::FfnBias: return ffn_pack_bias_launch(w, d32, st);
    case Pack::ChainLayer: return lin_chain_pack_launch(w, d.which, d.scale, d.lay, d16, st);
    case Pack::LinearT: return pack_linear_t_launch(w, d16, s.O, s.I, st, d.scale, d.ld);
    case Pack::Conv3Dgrad: return pack_conv3x3_dgrad_launch(w, d16, s.O, s.I, st);
    case Pack::Conv3S2Dgrad: return pack_conv3x3_s2_dgrad_launch(w, d16, s.O, s.I, st);
    case Pack::FlipOIHW: return flip_oihw_launch(w, d32, s.O, s.I, s.dims[2], st);
  }
  return HEDIT_ERR_STATE;
}

int store_load(ParamStore* h, const char* what, const char* name, const float* w, size_t numel, hipStream_t st) {
  h->finalized = false;
  auto it = h->index.find(name);
  if (it == h->index.end()) {
    hedit_set_error(std::string("unknown ") + what + (*what ? " " : "") + "parameter: " + name);
    return HEDIT_ERR_ARG;
  }
  ParamSlot& s = h->slots[it->second];
  if (s.numel != numel) {
    hedit_set_error(std::string("size mismatch for ") + name + ": expected " + std::to_string(s.numel) + ", got " + std::to_string(numel));
    return HEDIT_ERR_ARG;
  }
  TRY(pack(s, s.to, w, st));
  for (const PackDst& d : s.more) TRY(pack(s, d, w, st));
  s.loaded = true;
  return HEDIT_OK;
}

int store_missing(const ParamStore* h) {
  int m = 0;
  for (auto& s : h->slots) m += s.loaded ? 0 : 1;
  return m;
}
int store_num_params(const ParamStore* h) { return h ? (int)h->slots.size() : 0; }
const char* store_param_name(const ParamStore* h, int i) {
  if (!h || i < 0 || i >= (int)h->slots.size()) return nullptr;
  return h->slots[i].name.c_str();
}
int store_param_shape(const ParamStore* h, int i, int* ndim, int* dims4) {
  ARG_CHECK(h && ndim && dims4 && i >= 0 && i < (int)h->slots.size(), "param index");
  *ndim = h->slots[i].ndim;
  for (int k = 0; k < 4; ++k) dims4[k] = h->slots[i].dims[k];
  return HEDIT_OK;
}
int store_param_bf16_exact(const ParamStore* h, int i) {
  if (!h || i < 0 || i >= (int)h->slots.size()) return 0;
  const PackDst& d = h->slots[i].to;
  return (((d.kind == Pack::Linear || d.kind == Pack::ChainLayer) && d.scale == 1.f) || d.kind == Pack::Conv3 ||
          d.kind == Pack::GegluRows || d.kind == Pack::FfnLayer) ? 1 : 0;
}

int store_require_created(ParamStore* h, const char* fam) {
  if (!h->alloc_failed) return HEDIT_OK;
  hedit_set_error(std::string("hipMalloc failed while creating a hedit_") + fam + " handle");
  return HEDIT_ERR_HIP;
}
int store_require_loaded(const ParamStore* h, const char* what) {
  const int m = store_missing(h);
  if (m == 0) return HEDIT_OK;
  hedit_set_error(std::string(what) + " has " + std::to_string(m) + " unloaded parameters");
  return HEDIT_ERR_STATE;
}
int store_require_finalized(const ParamStore* h, const char* fam) {
  if (h->finalized) return HEDIT_OK;
  hedit_set_error(std::string("call hedit_") + fam + "_finalize after loading the parameters");
  return HEDIT_ERR_STATE;
}
