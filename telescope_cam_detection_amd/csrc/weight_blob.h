// weight_blob.h - the packed weight blob (weights.pack_blob: `RTDW`, a table of named fp32 tensors, 64-byte aligned payloads) as every
// handle that loads weights reads it: the detector engine, the ESRGAN upscaler, the EVA02 classifier and the YOLOX network.  One parser,
// which trusts no field of the table, and one scan of a tensor's values.  Which tensors a network needs, their shapes and the error codes
// of a missing one stay with each back end's own table check.  No HIP, no device: this header compiles on its own
// (tools/weight_blob_host_check.cpp runs it under -fsanitize=address,undefined).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "error.h"

namespace rtd {
namespace blob {

inline void need(bool ok, int code, const std::string& msg) {   // (the plain message: callers match on it)
  if (!ok) throw rtd::Error(code, msg);
}

struct HostTensor {
  const float* data = nullptr;
  std::vector<int64_t> shape;
  int64_t numel() const {
    int64_t n = 1;
    for (auto d : shape) n *= d;
    return n;
  }
};
inline void parse_blob(const char* b, size_t n, std::map<std::string, HostTensor>& out) {
  need(b && n >= 12 && memcmp(b, "RTDW", 4) == 0, RTD_E_WEIGHTS, "weight blob: bad magic");
  need(((uintptr_t)b & 3) == 0, RTD_E_WEIGHTS, "weight blob: not 4-byte aligned");
  uint32_t ver, count;
  memcpy(&ver, b + 4, 4);
  memcpy(&count, b + 8, 4);
  need(ver == 1, RTD_E_WEIGHTS, "weight blob: unsupported version");
  size_t p = 12;
  for (uint32_t i = 0; i < count; ++i) {
    need(n - p >= 2, RTD_E_WEIGHTS, "weight blob: truncated table");
    uint16_t nl;
    memcpy(&nl, b + p, 2); p += 2;
    need(n - p >= (size_t)nl + 4, RTD_E_WEIGHTS, "weight blob: truncated table");
    const std::string name(b + p, nl); p += nl;
    uint32_t nd;
    memcpy(&nd, b + p, 4); p += 4;
    need(nd <= 8 && n - p >= 4 * (size_t)nd + 16, RTD_E_WEIGHTS, "weight blob: truncated table");
    HostTensor t;
    const uint64_t cap = (uint64_t)1 << 40;   // elements of one tensor: checked before each multiply, so the product never wraps
    uint64_t numel = 1;
    for (uint32_t d = 0; d < nd; ++d) {
      uint32_t v;
      memcpy(&v, b + p, 4); p += 4;
      t.shape.push_back(v);
      need(v == 0 || numel <= cap / v, RTD_E_WEIGHTS, "weight blob: bad tensor extent: " + name);
      numel *= v;
    }
    uint64_t off, nb;
    memcpy(&off, b + p, 8); p += 8;
    memcpy(&nb, b + p, 8); p += 8;
    need(off % 4 == 0 && off <= n && nb <= n - off && nb == numel * 4, RTD_E_WEIGHTS, "weight blob: bad tensor extent: " + name);
    t.data = (const float*)(b + off);
    out[name] = t;
  }
}

// every value of tensor `name`: finite, and - pair engine - inside fp16's range (the hi half of a pair saturates at 65504)
inline void check_values(const std::string& name, const HostTensor& t, bool pair) {
  const int64_t n = t.numel();
  for (int64_t i = 0; i < n; ++i) {
    const float v = t.data[i];
    need(isfinite(v), RTD_E_WEIGHTS, "weight blob: tensor " + name + " holds a NaN or an infinity");
    need(!pair || fabsf(v) <= 65504.f, RTD_E_WEIGHTS,
         "weight blob: tensor " + name + " reaches " + std::to_string(v) + ", beyond the fp16 pair format's range (65504): use precision fp32");
  }
}

}  // namespace blob
}  // namespace rtd
