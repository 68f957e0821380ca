// Stand-alone check of the renderer's fill paths and restore-after-draw order
// (csrc/sim/raster.h), meant to be built with -fsanitize=address,undefined
// (tests/test_raster_fill_sanitized.py) and run once per fill path
// (BLENDTORCH_RASTER_ISA=scalar|avx2; the path in use is printed):
//   * incremental renders of the Cube scene into K = 3 rotating buffers (a
//     ring's life) at 100x75 and 64x48, 3 and 4 channels, both row orders,
//     each compared byte for byte against a full render of the same pose;
//   * the box is moved so that its silhouette and shadow leave the frame on
//     every side, are cut by it, and come back: the pieces of the previous
//     span that the new frame leaves uncovered then lie at the frame's edges,
//     and vector groups end at a row's last pixel;
//   * every buffer is an exactly sized heap block: a store past a span's row
//     or the buffer's end, or a restore that starts before it, is a report.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../sim/raster.h"

using namespace btn;

namespace {

struct Result {
  long frames = 0, mismatched = 0, edge_frames = 0;
};

void run(int W, int H, int C, bool lower_left, Result* res) {
  constexpr int K = 3;
  sim::Scene scene = sim::cube_scene();
  scene.cam.width = W, scene.cam.height = H;
  const size_t n = size_t(W) * H * size_t(C);
  sim::Renderer inc(scene, C, lower_left), full(scene, C, lower_left);
  std::vector<std::unique_ptr<uint8_t[]>> buf;
  for (int k = 0; k < K; ++k) {
    buf.emplace_back(new uint8_t[n]);
    std::memset(buf.back().get(), 0xa5, n);   // a slot that held anything
  }
  std::unique_ptr<uint8_t[]> ref(new uint8_t[n]);
  std::vector<sim::DirtyRect> dirty(K);
  std::mt19937_64 rng(uint64_t(W * 131 + C * 7 + (lower_left ? 1 : 0)));
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double pi = 3.14159265358979323846;
  // box centres: in the middle, cut by each side of the frame, outside it
  const double centres[][3] = {{0, 0, 0},   {3.5, 3.5, 0},  {-3.5, -3.5, 0}, {3.5, -3.5, 0}, {-3.5, 3.5, 0},
                               {0, 0, 2.5}, {5, 5, 0},      {-5, -5, 0},     {0, 0, 0},      {9, -9, 0},
                               {2, 2, 1},   {-6, 6, 0},     {6, -6, 1}};
  const int ncent = int(sizeof(centres) / sizeof(centres[0]));
  for (int i = 0; i < 4 * ncent; ++i) {
    sim::Box& b = scene.boxes[0];
    const double* c = centres[(i * 5) % ncent];   // consecutive frames of a buffer lie far apart and close
    b.center = {c[0] + 0.3 * U(rng), c[1] + 0.3 * U(rng), c[2]};
    b.rot = sim::euler_xyz(pi * U(rng), pi * U(rng), pi * U(rng));
    uint8_t* out = buf[size_t(i % K)].get();
    sim::DirtyRect& d = dirty[size_t(i % K)];
    inc.render(scene, out, &d);
    full.render(scene, ref.get());
    for (size_t k = 0; k < n; ++k) res->mismatched += out[k] != ref[k];
    res->frames++;
    if (!d.empty() && (d.x0 == 0 || d.y0 == 0 || d.x1 == W - 1 || d.y1 == H - 1)) res->edge_frames++;
  }
}

}  // namespace

int main() {
  Result res;
  const int sizes[][2] = {{100, 75}, {64, 48}};
  for (const auto& s : sizes)
    for (int C = 3; C <= 4; ++C)
      for (int ll = 0; ll < 2; ++ll) run(s[0], s[1], C, ll != 0, &res);
  const bool ok = res.mismatched == 0 && res.edge_frames > 0;
  std::printf("isa=%s frames=%ld edge_frames=%ld mismatched=%ld failed=%d\n", sim::raster_isa(), res.frames,
              res.edge_frames, res.mismatched, ok ? 0 : 1);
  return ok ? 0 : 1;
}
