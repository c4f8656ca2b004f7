// Stand-alone check of the pure host parts of the EVA02 classifier (csrc/classifier_host.h): config checks, the derived extents, the
// blob's tensor table against a well-formed blob (missing, mis-shaped, NaN and beyond-fp16 tensors; truncated blobs), and the arena layout
// of a plan (no two buffers overlap, every offset 256-byte aligned, sizes as the network needs them).
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/eva_host_check.cpp -o eva_host_check && ./eva_host_check
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "../telescope_cam_detection_amd/csrc/classifier_host.h"

namespace vh = eva_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

template <typename F>
static int code_of(F&& f) {
  try { f(); return RTD_OK; } catch (const rtd::Error& e) { return e.code; }
}

// weights.pack_blob of {name: fp32 tensor}
static std::vector<char> pack(const std::vector<vh::TensorDesc>& ts) {
  std::vector<char> head{'R', 'T', 'D', 'W'};
  auto put = [&](const void* p, size_t n) { head.insert(head.end(), (const char*)p, (const char*)p + n); };
  const uint32_t ver = 1, count = (uint32_t)ts.size();
  put(&ver, 4); put(&count, 4);
  size_t table = 0;
  for (auto& t : ts) table += 2 + t.name.size() + 4 + 4 * t.shape.size() + 16;
  uint64_t off = (head.size() + table + 63) / 64 * 64;
  std::vector<std::pair<uint64_t, uint64_t>> ext;
  for (auto& t : ts) {
    uint64_t n = 4;
    for (auto d : t.shape) n *= (uint64_t)d;
    ext.push_back({off, n});
    off = (off + n + 63) / 64 * 64;
  }
  for (size_t i = 0; i < ts.size(); ++i) {
    const uint16_t nl = (uint16_t)ts[i].name.size();
    put(&nl, 2); put(ts[i].name.data(), nl);
    const uint32_t nd = (uint32_t)ts[i].shape.size();
    put(&nd, 4);
    for (auto d : ts[i].shape) { const uint32_t v = (uint32_t)d; put(&v, 4); }
    put(&ext[i].first, 8); put(&ext[i].second, 8);
  }
  std::vector<char> blob(off, 0);
  memcpy(blob.data(), head.data(), head.size());
  for (size_t i = 0; i < ts.size(); ++i) {
    float* f = (float*)(blob.data() + ext[i].first);
    for (uint64_t k = 0; k < ext[i].second / 4; ++k) f[k] = 0.001f * (float)((k * 7 + i) % 97) - 0.04f;
  }
  return blob;
}

int main() {
  // ---- config: ViT-L/14 at 336 px, and the tests' tiny net
  rtd_eva_config big{(int32_t)sizeof(rtd_eva_config), 0, RTD_PREC_F16X3, 16, 336, 14, 1024, 24, 16, 2730, 10000, 16, 1, 1, RTD_EVA_POOL_TOKEN, 0};
  rtd_eva_config c{(int32_t)sizeof(rtd_eva_config), 0, RTD_PREC_F16X3, 3, 126, 14, 128, 2, 2, 341, 37, 16, 0, 0, RTD_EVA_POOL_AVG, 0};
  CHECK(code_of([&] { vh::check_config(&big); }) == RTD_OK && code_of([&] { vh::check_config(&c); }) == RTD_OK);
  auto bad = [&](auto edit) { rtd_eva_config d = c; edit(d); return code_of([&] { vh::check_config(&d); }); };
  CHECK(bad([](auto& d) { d.precision = RTD_PREC_BF16; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.heads = 4; }) == RTD_E_INVALID);             // head dim 32
  CHECK(bad([](auto& d) { d.img = 127; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.max_batch = 0; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.max_batch = 65; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.hidden = 4097; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.depth = 0; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.pool = 2; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.scale_mlp = 2; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.classes = 0; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.struct_size = 4; }) == RTD_E_INVALID);
  CHECK(code_of([&] { vh::check_config(nullptr); }) == RTD_E_INVALID);
  {
    const vh::Dims d = vh::dims(big);
    CHECK(d.G == 24 && d.L == 577 && d.Kp == 608 && d.Hp == 2752 && d.Cp == 10016);
    const vh::Dims t = vh::dims(c);
    CHECK(t.G == 9 && t.L == 82 && t.Kp == 608 && t.Hp == 352 && t.Cp == 64);
  }

  // ---- the arena of a plan: aligned, disjoint, of the network's sizes
  for (const rtd_eva_config* cfg : {&big, &c})
    for (int n : {1, 3, 16, 64}) {
      const vh::Layout a = vh::layout(*cfg, n);
      const vh::Dims d = vh::dims(*cfg);
      const size_t np = (size_t)n * d.G * d.G, nl = (size_t)n * d.L, D = cfg->dim;
      std::vector<std::pair<size_t, size_t>> bufs = {{a.patches, np * d.Kp * 4}, {a.pe, np * D * 4}, {a.xa, nl * D * 4}, {a.xb, nl * D * 4}, {a.y, nl * D * 4},
                                                     {a.qkv, nl * 3 * D * 4}, {a.ao, nl * D * 4}, {a.h1, nl * 2 * d.Hp * 4}, {a.h2, nl * d.Hp * 4},
                                                     {a.pool, n * D * 4}, {a.pooln, n * D * 4}, {a.logits, (size_t)n * d.Cp * 4}};
      std::sort(bufs.begin(), bufs.end());
      CHECK(bufs[0].first >= 256);
      for (size_t i = 0; i < bufs.size(); ++i) {
        CHECK(bufs[i].first % 256 == 0);
        CHECK(bufs[i].first + bufs[i].second <= (i + 1 < bufs.size() ? bufs[i + 1].first : a.top));
      }
    }
  CHECK(code_of([&] { vh::layout(c, 0); }) == RTD_E_INVALID && code_of([&] { vh::layout(c, 65); }) == RTD_E_INVALID);

  // ---- the tensor table and a blob that fits it
  const auto table = vh::tensor_table(c);
  CHECK(table.size() == 2 + 4 + 2u * 12 + 2 + 2);                        // per block: norm1, qkv, proj, norm2, fc1, fc2 (no inner LN, no mlp norm here)
  {
    rtd_eva_config both = c;
    both.scale_attn_inner = both.scale_mlp = 1;
    CHECK(vh::tensor_table(both).size() == table.size() + 2u * 4);
  }
  const std::vector<char> blob = pack(table);
  {
    std::map<std::string, vh::HostTensor> host;
    vh::parse_blob(blob.data(), blob.size(), host);
    CHECK(host.size() == table.size());
    vh::check_tensors(host, table, true);
    CHECK((host.at("blocks.1.mlp.fc1.weight").shape == std::vector<int64_t>{704, 128}));
    CHECK((host.at("rope_sin").shape == std::vector<int64_t>{81, 64}));
    auto h2 = host;
    h2.erase("blocks.0.attn.qkv.bias");
    CHECK(code_of([&] { vh::check_tensors(h2, table, true); }) == RTD_E_WEIGHTS);
    h2 = host;
    h2["pos_embed"].shape = {81, 128};
    CHECK(code_of([&] { vh::check_tensors(h2, table, true); }) == RTD_E_WEIGHTS);
    // the same blob against another architecture's table
    rtd_eva_config other = c;
    other.scale_mlp = 1;
    CHECK(code_of([&] { vh::check_tensors(host, vh::tensor_table(other), true); }) == RTD_E_WEIGHTS);
  }
  {
    std::vector<char> b2 = blob;
    std::map<std::string, vh::HostTensor> host;
    vh::parse_blob(b2.data(), b2.size(), host);
    float* w = (float*)host.at("head.weight").data;
    w[100] = 70000.f;
    CHECK(code_of([&] { vh::check_tensors(host, table, true); }) == RTD_E_WEIGHTS);
    CHECK(code_of([&] { vh::check_tensors(host, table, false); }) == RTD_OK);
    w[100] = NAN;
    CHECK(code_of([&] { vh::check_tensors(host, table, false); }) == RTD_E_WEIGHTS);
  }
  // truncations: refused, never read past the end (exact-size heap copies)
  const size_t table_end = 12 + [&] { size_t n = 0; for (auto& t : table) n += 2 + t.name.size() + 4 + 4 * t.shape.size() + 16; return n; }();
  for (size_t n = 0; n < blob.size(); n += (n < table_end + 8 ? 1 : 65521)) {
    char* cut = (char*)malloc(n ? n : 1);
    memcpy(cut, blob.data(), n);
    std::map<std::string, vh::HostTensor> host;
    CHECK(code_of([&] { vh::parse_blob(cut, n, host); }) == RTD_E_WEIGHTS);
    free(cut);
  }
  printf("eva host check ok\n");
  return 0;
}
