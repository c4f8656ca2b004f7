// Stand-alone check of the packed weight blob's parser and value scan (csrc/weight_blob.h), the one every handle that loads weights
// reads its blob with: well-formed blobs, blobs truncated at every length, corrupted table fields, table fields crafted to pass a check
// that adds before it compares (offsets and sizes that wrap 64 bits, extents whose product does), a misaligned base, and the scan's
// limits.  Every blob lies in a heap block of its exact size, so a read past either end is a sanitizer report.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/weight_blob_host_check.cpp -o weight_blob_host_check && ./weight_blob_host_check
#include <stdio.h>
#include <stdlib.h>

#include "../telescope_cam_detection_amd/csrc/weight_blob.h"

namespace wb = rtd::blob;
typedef std::map<std::string, wb::HostTensor> Host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

template <typename F>
static int code_of(F&& f) {
  try { f(); return RTD_OK; } catch (const rtd::Error& e) { return e.code; }
}
template <typename F>
static std::string message_of(F&& f) {
  try { f(); return ""; } catch (const rtd::Error& e) { return e.what(); }
}

// one table entry as written: nothing about it is made consistent
struct Entry {
  std::string name;
  std::vector<uint32_t> dims;
  uint64_t off, nb;
  uint16_t name_len_field;   // what the table says the name's length is
  uint32_t nd_field;         // what the table says the number of extents is
};
static Entry entry(const std::string& name, const std::vector<uint32_t>& dims, uint64_t off, uint64_t nb) {
  return Entry{name, dims, off, nb, (uint16_t)name.size(), (uint32_t)dims.size()};
}
static size_t table_bytes(const std::vector<Entry>& es) {
  size_t n = 12;
  for (const Entry& e : es) n += 2 + e.name.size() + 4 + 4 * e.dims.size() + 16;
  return n;
}
// `total` bytes: magic, version, count, the entries, zeros behind them
static std::vector<char> raw(const std::vector<Entry>& es, size_t total, uint32_t ver = 1) {
  std::vector<char> b{'R', 'T', 'D', 'W'};
  auto put = [&](const void* p, size_t n) { b.insert(b.end(), (const char*)p, (const char*)p + n); };
  const uint32_t count = (uint32_t)es.size();
  put(&ver, 4); put(&count, 4);
  for (const Entry& e : es) {
    put(&e.name_len_field, 2); put(e.name.data(), e.name.size());
    put(&e.nd_field, 4);
    for (uint32_t d : e.dims) put(&d, 4);
    put(&e.off, 8); put(&e.nb, 8);
  }
  CHECK(b.size() <= total);
  b.resize(total, 0);
  return b;
}
// weights.pack_blob of {name: shape}: 64-byte aligned payloads behind the table, tensor i filled with a pattern of (i, k)
static float pattern(size_t i, uint64_t k) { return 0.001f * (float)((k * 7 + i) % 97) - 0.04f; }
static std::vector<char> pack(const std::vector<std::pair<std::string, std::vector<uint32_t>>>& ts) {
  std::vector<Entry> es;
  for (auto& t : ts) es.push_back(entry(t.first, t.second, 0, 0));
  uint64_t off = (table_bytes(es) + 63) / 64 * 64;
  for (Entry& e : es) {
    e.nb = 4;
    for (uint32_t d : e.dims) e.nb *= d;
    e.off = off;
    off = (off + e.nb + 63) / 64 * 64;
  }
  std::vector<char> blob = raw(es, off);
  for (size_t i = 0; i < es.size(); ++i)
    for (uint64_t k = 0; k < es[i].nb / 4; ++k) ((float*)(blob.data() + es[i].off))[k] = pattern(i, k);
  return blob;
}
// parse an exact-size heap copy of b[0, n) placed `shift` bytes into its block; the code of the refusal (RTD_OK: parsed, and every
// tensor's first and last value read)
static int parse_copy(const std::vector<char>& b, size_t n, Host* out = nullptr, size_t shift = 0) {
  char* block = (char*)malloc(n + shift ? n + shift : 1);
  memcpy(block + shift, b.data(), n);
  Host host;
  const int code = code_of([&] { wb::parse_blob(block + shift, n, host); });
  if (code == RTD_OK)
    for (const auto& kv : host)
      if (kv.second.numel() > 0) { volatile float a = kv.second.data[0], z = kv.second.data[kv.second.numel() - 1]; (void)a; (void)z; }
  if (out) {   // (the data pointers die with the block: only names and shapes are looked at afterwards)
    *out = host;
    for (auto& kv : *out) kv.second.data = nullptr;
  }
  free(block);
  return code;
}

int main() {
  // ---- well formed
  const std::vector<std::pair<std::string, std::vector<uint32_t>>> ts = {
      {"conv_first.weight", {64, 3, 3, 3}}, {"conv_first.bias", {64}}, {"scalar", {}}, {"empty", {0, 5}}, {"pos_embed", {17, 64}}, {"", {16}}};   // (the last payload ends where the blob does)
  const std::vector<char> blob = pack(ts);
  {
    Host host;
    wb::parse_blob(blob.data(), blob.size(), host);
    CHECK(host.size() == ts.size());
    for (size_t i = 0; i < ts.size(); ++i) {
      const wb::HostTensor& t = host.at(ts[i].first);
      CHECK(t.shape == std::vector<int64_t>(ts[i].second.begin(), ts[i].second.end()));
      CHECK((const char*)t.data >= blob.data() && (const char*)(t.data + t.numel()) <= blob.data() + blob.size());
      CHECK(((uintptr_t)t.data & 3) == 0);
      for (int64_t k = 0; k < t.numel(); ++k) CHECK(t.data[k] == pattern(i, (uint64_t)k));
      wb::check_values(ts[i].first, t, true);
    }
    CHECK(host.at("scalar").numel() == 1 && host.at("empty").numel() == 0 && host.at("pos_embed").numel() == 17 * 64);
  }
  CHECK(parse_copy(blob, blob.size()) == RTD_OK);
  CHECK(parse_copy(raw({}, 12), 12) == RTD_OK);                         // an empty table
  // the header
  CHECK(code_of([&] { Host h; wb::parse_blob(nullptr, 64, h); }) == RTD_E_WEIGHTS);
  { std::vector<char> b2 = blob; b2[0] = 'X'; CHECK(parse_copy(b2, b2.size()) == RTD_E_WEIGHTS); }
  CHECK(parse_copy(raw({}, 64, 2), 64) == RTD_E_WEIGHTS);
  CHECK(message_of([&] { Host h; wb::parse_blob(blob.data(), 11, h); }) == "weight blob: bad magic");
  // a misaligned base pointer: refused before a float pointer into it exists
  for (size_t shift : {1, 2, 3}) CHECK(parse_copy(blob, blob.size(), nullptr, shift) == RTD_E_WEIGHTS);
  { char* block = (char*)malloc(blob.size() + 1);
    memcpy(block + 1, blob.data(), blob.size());
    CHECK(message_of([&] { Host h; wb::parse_blob(block + 1, blob.size(), h); }) == "weight blob: not 4-byte aligned");
    free(block); }

  // ---- every truncation of the table region and a sweep of longer ones: refused, never read past the end
  const size_t table_end = [&] { std::vector<Entry> es; for (auto& t : ts) es.push_back(entry(t.first, t.second, 0, 0)); return table_bytes(es); }();
  for (size_t n = 0; n < blob.size(); n += (n < table_end + 8 ? 1 : 61))
    CHECK(parse_copy(blob, n) == RTD_E_WEIGHTS);      // every tensor's extent must lie inside the blob: only the full length parses
  // ---- corrupted table bytes: any outcome but a bad access
  for (size_t i = 4; i < table_end; ++i)
    for (unsigned char v : {0x00, 0xff, 0x7f, 0x80}) {
      std::vector<char> b2 = blob;
      b2[i] = (char)v;
      const int code = parse_copy(b2, b2.size());
      CHECK(code == RTD_OK || code == RTD_E_WEIGHTS);
    }

  // ---- fields that pass `off + nb <= n` or `p + len <= n` only because the sum wraps
  const size_t N = 256;
  auto refused = [&](const Entry& e, const char* what) {
    const std::vector<char> b = raw({e}, N);
    Host host;
    const std::string msg = message_of([&] { Host h; wb::parse_blob(b.data(), b.size(), h); });
    CHECK(parse_copy(b, b.size(), &host) == RTD_E_WEIGHTS && host.empty());
    CHECK(msg.find(what) != std::string::npos);
  };
  CHECK(parse_copy(raw({entry("t", {2}, 64, 8)}, N), N) == RTD_OK);                  // (the well-formed neighbour of the cases below)
  CHECK(parse_copy(raw({entry("t", {2}, N - 8, 8)}, N), N) == RTD_OK);               // the last 8 bytes
  CHECK(parse_copy(raw({entry("t", {0}, N, 0)}, N), N) == RTD_OK);                   // nothing, at the end
  refused(entry("t", {2}, ~(uint64_t)0 - 3, 8), "bad tensor extent");                // off = 2^64 - 4: off + nb = 4
  refused(entry("t", {2}, N - 4, 8), "bad tensor extent");                           // leaves the blob by 4 bytes
  refused(entry("t", {2}, N - 4, ~(uint64_t)0 - 3), "bad tensor extent");            // off just below n, off + nb = n - 8
  refused(entry("t", {0x40000000u, 2}, N - 4, (uint64_t)1 << 33), "bad tensor extent");   // a size that is its extents' but not in the blob
  refused(entry("t", {0}, N + 4, 0), "bad tensor extent");                           // an empty tensor outside
  refused(entry("t", {2}, 66, 8), "bad tensor extent");                              // off % 4
  refused(entry("t", {3}, 64, 8), "bad tensor extent");                              // nb != 4 numel
  // eight extents whose product wraps 64 bits to 0, to 2, to 2^62 (a signed product: negative before the * 4)
  refused(entry("t", {65536, 65536, 65536, 65536, 1, 1, 1, 1}, 64, 0), "bad tensor extent");
  refused(entry("t", {0x80000000u, 0x80000000u, 4, 1, 1, 1, 1, 2}, 64, 8), "bad tensor extent");
  refused(entry("t", {0x80000000u, 0x80000000u, 1, 1, 1, 1, 1, 1}, 64, 0), "bad tensor extent");
  refused(entry("t", {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, 64, 4), "bad tensor extent");
  refused(entry("t", {1u << 20, 1u << 20, 2}, 64, 8), "bad tensor extent");          // 2^41 elements: past the cap, no wrap needed
  // a running product AT the cap times an extent that wraps it: exactly 2^64 (-> 0), 2^64 + 2^40, and 2^40 x (2^32 - 1)
  refused(entry("t", {1u << 20, 1u << 20, 1u << 24}, 64, 0), "bad tensor extent");
  refused(entry("t", {1u << 20, 1u << 20, (1u << 24) + 1}, 64, (uint64_t)1 << 42), "bad tensor extent");
  refused(entry("t", {1u << 20, 1u << 20, 0xffffffffu}, 64, 0), "bad tensor extent");
  refused(entry("t", {1u << 20, 1u << 20, 1, 1u << 24, 0, 7}, 64, 0), "bad tensor extent");   // (a later zero extent does not excuse it)
  CHECK(parse_copy(raw({entry("t", {0, 0xffffffffu, 0xffffffffu, 0xffffffffu}, 64, 0)}, N), N) == RTD_OK);   // zero first: every product is 0
  // a name length and a number of extents that run past the end
  { Entry e = entry("t", {2}, 64, 8); e.name_len_field = 0xffff; refused(e, "truncated table"); }
  { Entry e = entry("t", {2}, 64, 8); e.name_len_field = (uint16_t)(N - 14); refused(e, "truncated table"); }   // the name ends where the blob does
  { Entry e = entry("t", {2}, 64, 8); e.nd_field = 9; refused(e, "truncated table"); }
  { Entry e = entry("t", {2}, 64, 8); e.nd_field = 0xffffffffu; refused(e, "truncated table"); }                 // 4 * nd wraps 32 bits
  { Entry e = entry("t", {2}, 64, 8); e.nd_field = 0x40000001u; refused(e, "truncated table"); }
  { const std::vector<char> b = raw({entry("name", {1, 2, 3, 4, 5, 6, 7, 8}, 0, 0)}, 12 + 2 + 4 + 4 + 32 + 16);   // nd = 8, cut one byte short of its sizes
    CHECK(parse_copy(b, b.size() - 1) == RTD_E_WEIGHTS); }
  { std::vector<char> b = raw({}, 12); uint32_t count = 0xffffffffu; memcpy(b.data() + 8, &count, 4);            // a count with no table behind it
    CHECK(parse_copy(b, b.size()) == RTD_E_WEIGHTS); }

  // ---- the value scan
  {
    const std::vector<char> b = pack({{"w", {4, 8}}});
    std::vector<char> copy = b;
    Host host;
    wb::parse_blob(copy.data(), copy.size(), host);
    const wb::HostTensor& t = host.at("w");
    float* w = (float*)t.data;
    const float above = nextafterf(65504.f, INFINITY);
    CHECK(above > 65504.f);
    for (bool pair : {false, true}) CHECK(code_of([&] { wb::check_values("w", t, pair); }) == RTD_OK);
    for (float edge : {65504.f, -65504.f}) {
      w[31] = edge;                                                  // the last value: the scan reaches it
      for (bool pair : {false, true}) CHECK(code_of([&] { wb::check_values("w", t, pair); }) == RTD_OK);
    }
    for (float big : {above, -above, 70000.f, 3.0e38f}) {
      w[31] = big;
      CHECK(code_of([&] { wb::check_values("w", t, true); }) == RTD_E_WEIGHTS);
      CHECK(message_of([&] { wb::check_values("w", t, true); }).find("weight blob: tensor w reaches ") == 0);
      CHECK(code_of([&] { wb::check_values("w", t, false); }) == RTD_OK);
    }
    w[31] = 0.f;
    for (float bad : {NAN, INFINITY, -INFINITY})
      for (int at : {0, 13, 31}) {
        w[at] = bad;
        for (bool pair : {false, true}) {
          CHECK(code_of([&] { wb::check_values("w", t, pair); }) == RTD_E_WEIGHTS);
          CHECK(message_of([&] { wb::check_values("w", t, pair); }) == "weight blob: tensor w holds a NaN or an infinity");
        }
        w[at] = 0.f;
      }
    wb::HostTensor none;                                             // no extents, no data: one element would be read - an empty one reads nothing
    none.shape = {0};
    wb::check_values("none", none, true);
  }
  printf("weight blob host check ok\n");
  return 0;
}
