// Stand-alone check of the back ends' host scaffold (csrc/backend.h) on a machine WITHOUT a GPU: every HIP call fails there, which is
// the path to exercise - a handle that was only partly built is destroyed once and leaks nothing, exceptions become return codes and
// messages, and a buffer whose allocation failed stays empty.  CPU only: build and run it where no device is visible.
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/backend_host_check.cpp -o backend_host_check && ./backend_host_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>

#include "../telescope_cam_detection_amd/csrc/backend.h"

namespace bk = rtd::backend;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

struct Dummy : bk::Base {
  bk::OwnStream q;
  bk::PinBuf pin;
  bk::DevBuf dev;
  int* extra = nullptr;
};
struct Other : bk::Base {};

static int destroyed = 0;
static void destroy(Dummy* h) {
  if (!h) return;
  ++destroyed;
  h->q.drain();
  h->dev.release();
  h->pin.release();
  h->q.close();
  delete[] h->extra;
  delete h;
}

int main() {
  int count = 0;
  if (hipGetDeviceCount(&count) == hipSuccess && count > 0) {
    printf("backend host check skipped: a GPU is visible (this check is for the failure paths of a machine without one)\n");
    return 0;
  }
  (void)hipGetLastError();

  // ---- a create whose init throws after a partial build: destroyed once, *out null, the message kept for last_error(NULL)
  Dummy* h = (Dummy*)0x1;
  int rc = bk::create(&h, destroy, [&](Dummy* x) {
    x->extra = new int[16];
    bk::use_device(0);        // no device: throws
    x->q.open();
  });
  CHECK(rc == RTD_E_HIP || rc == RTD_E_INVALID);
  CHECK(h == nullptr && destroyed == 1);
  CHECK(strlen(bk::last_error<Dummy>(nullptr)) > 0);
  CHECK(strlen(bk::last_error<Other>(nullptr)) == 0);                 // one string per handle type
  {
    bool empty_elsewhere = false;
    std::thread t([&] { empty_elsewhere = strlen(bk::last_error<Dummy>(nullptr)) == 0; });
    t.join();
    CHECK(empty_elsewhere);                                           // and per thread
  }
  CHECK(bk::create((Dummy**)nullptr, destroy, [](Dummy*) {}) == RTD_E_INVALID);

  // ---- bad_alloc and a refusal inside init
  rc = bk::create(&h, destroy, [](Dummy*) { throw std::bad_alloc(); });
  CHECK(rc == RTD_E_OOM && h == nullptr && destroyed == 2 && strcmp(bk::last_error<Dummy>(nullptr), "host allocation failed") == 0);
  rc = bk::create(&h, destroy, [](Dummy*) { RTD_CHECK(false, RTD_E_INVALID, "blur_size must be odd"); });
  CHECK(rc == RTD_E_INVALID && h == nullptr && destroyed == 3 && strstr(bk::last_error<Dummy>(nullptr), "blur_size must be odd"));
  rc = bk::create(&h, destroy, [](Dummy*) { throw std::runtime_error("other"); });
  CHECK(rc == RTD_E_HIP && h == nullptr && destroyed == 4 && strcmp(bk::last_error<Dummy>(nullptr), "other") == 0);

  // ---- a handle that needs no device
  rc = bk::create(&h, destroy, [](Dummy* x) { x->extra = new int[4]; });
  CHECK(rc == RTD_OK && h != nullptr && destroyed == 4);
  CHECK(strlen(bk::last_error(h)) == 0);

  // ---- guarded: the code and the message of what the call threw; a null handle
  rc = bk::guarded(h, [&] { RTD_CHECK(false, RTD_E_STATE, "refused"); });
  CHECK(rc == RTD_E_STATE && strncmp(bk::last_error(h), "refused", 7) == 0);
  rc = bk::guarded(h, [&] { throw std::bad_alloc(); });
  CHECK(rc == RTD_E_OOM && strcmp(bk::last_error(h), "host allocation failed") == 0);
  CHECK(bk::guarded(h, [] {}) == RTD_OK);
  CHECK(bk::guarded((Dummy*)nullptr, [] {}) == RTD_E_INVALID);

  // ---- a failed reserve leaves the buffer empty, and release() of an empty buffer does nothing
  rc = bk::guarded(h, [&] { h->dev.reserve(64); });
  CHECK(rc != RTD_OK && h->dev.p == nullptr && h->dev.cap == 0 && strlen(bk::last_error(h)) > 0);
  rc = bk::guarded(h, [&] { h->pin.reserve(64); });
  CHECK(rc != RTD_OK && h->pin.p == nullptr && h->pin.cap == 0);
  h->dev.reserve(0);                                                  // nothing asked for: no allocation, no throw
  h->dev.release();
  h->pin.release();
  CHECK(h->dev.p == nullptr && h->pin.p == nullptr);

  // ---- a stream that cannot be opened stays closed; drain / close of a closed one do nothing
  rc = bk::guarded(h, [&] { h->q.open(); });
  CHECK(rc != RTD_OK && h->q.stream == nullptr && h->q.ev_xs == nullptr);
  h->q.drain();
  h->q.close();

  // ---- the scratch of one call: a failed get / event / stream throws and leaves nothing held; what is held goes exactly once (release
  // empties the lists, so the destructor after it - and a second release - frees nothing; there is no copy that could free it again)
  static_assert(!std::is_copy_constructible<bk::OpScratch>::value && !std::is_copy_assignable<bk::OpScratch>::value, "one owner");
  {
    bk::OpScratch sc;
    std::string err;
    CHECK(bk::caught(err, [&] { sc.get<float>(64); }) != RTD_OK && err.find("hipMalloc") != std::string::npos);
    CHECK(bk::caught(err, [&] { sc.zeros<float>(64); }) != RTD_OK);
    const float one = 1.f;
    CHECK(bk::caught(err, [&] { sc.upload(&one, 1); }) != RTD_OK);
    CHECK(bk::caught(err, [&] { sc.event(); }) != RTD_OK && err.find("hipEventCreate") != std::string::npos);
    CHECK(bk::caught(err, [&] { sc.stream(); }) != RTD_OK);
    CHECK(sc.bufs.empty() && sc.events.empty() && sc.streams.empty());
    sc.release();                                                       // empty: frees nothing
    CHECK(sc.bufs.empty() && sc.events.empty() && sc.streams.empty());
    // (no device: hipFree refuses the address without touching it)
    sc.bufs.push_back((void*)0x1000);
    sc.release();
    CHECK(sc.bufs.empty());
    sc.release();
  }
  rc = bk::guarded(h, [&] {                                             // a throw past a scratch that holds something unwinds through its destructor
    bk::OpScratch sc;
    sc.bufs.push_back((void*)0x1000);
    RTD_CHECK(false, RTD_E_INVALID, "refused after staging");
  });
  CHECK(rc == RTD_E_INVALID && strncmp(bk::last_error(h), "refused after staging", 21) == 0);

  // ---- the padded extents of a conv filter against the kernels' three padding formulas, and the host-side row padding
  for (int K : {27, 64, 576, 2304 + 256})
    for (int N : {3, 32, 80, 256, 300}) {
      const int kpad = (K + 63) / 64 * 64, npad = (N + 127) / 128 * 128, kpad_split = 2 * ((K + 31) / 32 * 32);
      for (int dt : {(int)rtd::BF16, (int)rtd::F32, (int)rtd::F16X2}) {
        const rtd::ConvFilter f = rtd::conv_filter_extents(dt, N, K);
        CHECK(f.N == N && f.K == K && f.dt == dt && f.w == nullptr && f.bias == nullptr);
        CHECK(f.Npad == npad && f.Kpad == (dt == rtd::F16X2 ? kpad_split : kpad));
        CHECK(f.kcols() == (dt == rtd::F16X2 ? kpad_split / 2 : kpad));
        CHECK(f.bytes() == (size_t)npad * f.Kpad * (dt == rtd::F32 ? 4 : 2));
        CHECK(f.kcols() >= K && f.kcols() % 32 == 0 && f.bytes() % 512 == 0);
      }
    }
  {
    // two segments side by side along K (a block's last conv with its projection shortcut): [N][K1 | K2], zero padded to [Npad][kcols]
    const int N = 3, K1 = 5, K2 = 27;
    std::vector<float> w1((size_t)N * K1), w2((size_t)N * K2);
    for (size_t i = 0; i < w1.size(); ++i) w1[i] = 1.f + (float)i;
    for (size_t i = 0; i < w2.size(); ++i) w2[i] = -1.f - (float)i;
    for (int dt : {(int)rtd::BF16, (int)rtd::F16X2}) {
      const rtd::ConvFilter f = rtd::conv_filter_extents(dt, N, K1 + K2);
      const std::vector<float> rows = rtd::conv_filter_rows(f, {{w1.data(), K1}, {w2.data(), K2}});
      CHECK(rows.size() == (size_t)f.Npad * f.kcols());
      for (int r = 0; r < f.Npad; ++r)
        for (int k = 0; k < f.kcols(); ++k) {
          const float want = r >= N || k >= K1 + K2 ? 0.f : (k < K1 ? w1[(size_t)r * K1 + k] : w2[(size_t)r * K2 + k - K1]);
          CHECK(rows[(size_t)r * f.kcols() + k] == want);
        }
    }
  }

  // ---- the staged-frame offsets and the shared crop checks
  {
    const int32_t hwc[6] = {2, 3, 3, 1, 1, 1};
    std::vector<size_t> foff;
    CHECK(bk::stage_offsets(2, hwc, false, 512, foff) == 512 + 256 + 256 && foff[0] == 512 && foff[1] == 768);
    CHECK(bk::stage_offsets(2, hwc, true, 512, foff) == 512 && foff[0] == 512 && foff[1] == 512);
    CHECK(bk::align_up(0, 256) == 0 && bk::align_up(1, 256) == 256 && bk::align_up(256, 256) == 256);
    const uint8_t px = 0;
    const uint8_t* frames[1] = {&px};
    const uint8_t* none[1] = {nullptr};
    const int32_t hw[2] = {32, 32}, inside[4] = {0, 0, 16, 16}, outside[4] = {0, 0, 33, 16};
    uint8_t out = 0;
    CHECK(bk::guarded(h, [&] { bk::check_crop_call(1, frames, hw, inside, &out); bk::check_crop_frame(0, frames, hw, inside); }) == RTD_OK);
    CHECK(bk::guarded(h, [&] { bk::check_crop_call(0, frames, hw, inside, &out); }) == RTD_E_INVALID && strstr(bk::last_error(h), "1..64 crops per call"));
    CHECK(bk::guarded(h, [&] { bk::check_crop_call(1, frames, hw, inside, nullptr); }) == RTD_E_INVALID && strstr(bk::last_error(h), "null argument"));
    CHECK(bk::guarded(h, [&] { bk::check_crop_frame(0, none, hw, inside); }) == RTD_E_INVALID && strstr(bk::last_error(h), "crop 0 has a null frame"));
    CHECK(bk::guarded(h, [&] { bk::check_crop_frame(0, frames, hw, outside); }) == RTD_E_INVALID && strstr(bk::last_error(h), "crop 0 leaves its frame"));
  }

  destroy(h);
  CHECK(destroyed == 5);
  destroy(nullptr);
  CHECK(destroyed == 5);
  printf("backend host check ok\n");
  return 0;
}
