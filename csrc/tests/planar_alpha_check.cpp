// Stand-alone check of the rgb_a slot layout (csrc/common/planar_alpha.h),
// meant to be built with -fsanitize=address,undefined (tests/test_planar_alpha_sanitized.py):
//   * render equality: 200 random poses rendered incrementally (DirtyRect) by
//     the 3-channel renderer into ONE planar buffer, the alpha plane filled
//     once; after every pose the buffer, re-interleaved with the helper, must
//     equal a fresh full 4-channel render -- both row orders;
//   * bounds: interleave_rgb_a and rgb_a_valid on exact-size heap buffers;
//   * the ring header: hint bits through Segment, and a version-1 header refused.
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../common/planar_alpha.h"
#include "../sim/raster.h"
#include "../transport/shmring.h"

using namespace btn;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++g_failed;                                                       \
    }                                                                   \
  } while (0)

long render_equality(bool lower_left, int poses) {
  sim::Scene scene = sim::cube_scene();
  scene.cam.width = 320, scene.cam.height = 240;   // box spans still cross the renderer's 64-pixel chunks
  const int W = scene.cam.width, H = scene.cam.height;
  const size_t npix = size_t(W) * H;
  sim::Renderer rgb(scene, 3, lower_left), rgba(scene, 4, lower_left);
  // exact-size heap buffers: a write past either end is an ASan report
  std::unique_ptr<uint8_t[]> slot(new uint8_t[npix * 4]), relaid(new uint8_t[npix * 4]), full(new uint8_t[npix * 4]);
  std::memset(slot.get(), 0x5a, npix * 4);   // a slot that held anything
  sim::DirtyRect dirty;
  std::mt19937_64 rng(lower_left ? 11 : 5);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double pi = 3.14159265358979323846;
  long mismatched = 0;
  for (int i = 0; i < poses; ++i) {
    scene.boxes[0].rot = sim::euler_xyz(pi * U(rng), pi * U(rng), pi * U(rng));
    if (!dirty.known) std::memset(slot.get() + npix * 3, 255, npix);   // unknown content: alpha once
    rgb.render(scene, slot.get(), &dirty);
    planar::interleave_rgb_a(relaid.get(), slot.get(), slot.get() + npix * 3, npix);
    rgba.render(scene, full.get());
    if (std::memcmp(relaid.get(), full.get(), npix * 4) != 0)
      for (size_t k = 0; k < npix * 4; ++k) mismatched += relaid[k] != full[k];
  }
  return mismatched;
}

void bounds(int h, int w) {
  const size_t npix = size_t(h) * w;
  std::unique_ptr<uint8_t[]> rgb(new uint8_t[npix * 3]), a(new uint8_t[npix]), dst(new uint8_t[npix * 4]);
  for (size_t i = 0; i < npix * 3; ++i) rgb[i] = uint8_t(i * 7 + 1);
  for (size_t i = 0; i < npix; ++i) a[i] = uint8_t(200 + i);
  planar::interleave_rgb_a(dst.get(), rgb.get(), a.get(), npix);
  for (size_t p = 0; p < npix; ++p) {
    CHECK(dst[4 * p] == rgb[3 * p] && dst[4 * p + 1] == rgb[3 * p + 1] && dst[4 * p + 2] == rgb[3 * p + 2]);
    CHECK(dst[4 * p + 3] == a[p]);
  }
  // a frame that ends exactly at its slot's end is valid, one byte further is not
  const uint64_t bytes = uint64_t(npix) * 4;
  CHECK(planar::rgb_a_valid(h, w, 4096, 4096 + bytes));
  CHECK(!planar::rgb_a_valid(h, w, 4097, 4096 + bytes));
  CHECK(!planar::rgb_a_valid(h, w, 4096, 4096 + bytes - 1));
  CHECK(!planar::rgb_a_valid(h, w, -16, bytes));
  CHECK(!planar::rgb_a_valid(h, w, 4096, 0));
}

void ring_header() {
  const std::string name = "blendtorch-" + std::to_string(::getpid()) + "-planar-check";
  {
    std::unique_ptr<shm::Segment> prod(shm::Segment::create(name, 2, 4096));
    std::unique_ptr<shm::Segment> cons(shm::Segment::open(name));
    CHECK(prod->hint() == 0);
    cons->add_hint(shm::kWantPlanarAlpha);
    CHECK(prod->hint() == shm::kWantPlanarAlpha);
    cons->add_hint(shm::kNeedInterleaved);
    cons->add_hint(shm::kWantPlanarAlpha);
    CHECK(prod->hint() == (shm::kWantPlanarAlpha | shm::kNeedInterleaved));   // OR-ed and sticky
    const int s = prod->acquire(0);
    CHECK(s == 0 && prod->publish(uint32_t(s)) == 1 && cons->claim(0, 1));   // the slot words moved behind the hint
    cons->release(0, 1);
    CHECK(prod->free_count() == 2);
  }
  // a version-1 ring (32-byte header, no hint word) is refused
  const std::string path = "/" + name + "-v1";
  const int fd = ::shm_open(path.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
  CHECK(fd >= 0 && ::ftruncate(fd, 8192) == 0);
  void* p = ::mmap(nullptr, 8192, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  CHECK(p != MAP_FAILED);
  auto* h = static_cast<shm::Header*>(p);
  h->magic = shm::kMagic, h->version = 1, h->nslots = 1, h->slot_bytes = 4096, h->data_offset = 4096;
  bool refused = false;
  try {
    std::unique_ptr<shm::Segment> old(shm::Segment::open(path));
  } catch (const std::runtime_error& e) {
    refused = std::strstr(e.what(), "version 1") != nullptr;
  }
  CHECK(refused);
  ::munmap(p, 8192);
  ::close(fd);
  ::shm_unlink(path.c_str());
}

}  // namespace

int main() {
  const long up = render_equality(false, 200), low = render_equality(true, 200);
  CHECK(up == 0 && low == 0);
  bounds(8, 32);
  bounds(8, 6);
  CHECK(!planar::supported(3, 4, 4));                                   // 36 bytes of RGB: alpha plane unaligned
  CHECK(!planar::supported(8, 32, 3) && !planar::supported(0, 32, 4));
  CHECK(!planar::rgb_a_valid(int64_t(1) << 40, int64_t(1) << 40, 0, ~uint64_t(0)));   // no overflow into "valid"
  ring_header();
  std::printf("mismatched_upper=%ld mismatched_lower=%ld failed=%d\n", up, low, g_failed);
  return g_failed == 0 ? 0 : 1;
}
