// texts_states_harness -- asks recur_amd/csrc/texts_states.h (with texts_plan.h's order) without a GPU, for
// tests/test_texts_states.py.  Built with g++ alone; the same program is built again under the sanitizers.
//
//   texts_states_harness WAVE_WIDTH WIDTH HIDDEN MODE LEN,LEN,...
//
// MODE: "sep" (h_out an array of its own), "inplace" (h_out is h_in), "null" (h_in NULL: every row from the fallback
// row).  The states are h_in[k][i] = 1000 k + i, the fallback row is -1 - i, h_out and the staging buffer start as -7777.
// Every wave is packed, "run" -- the device's part, here: 0.5 added to the elements [1, HIDDEN] of every staged row, so
// that a state that went through a wave differs from one that was filled --, and unpacked; then the texts without a row
// are filled.  Written to stdout as raw float32: what every wave's pack left in the staging buffer, wave after wave
// ([n_rows][WIDTH]); h_out ([n_texts][WIDTH]); h_in as it is afterwards ([n_texts][WIDTH]; for "null" nothing).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "texts_states.h"

int main(int argc, char **argv) {
  if (argc != 6) return 2;
  const int wave_width = atoi(argv[1]), width = atoi(argv[2]), hidden = atoi(argv[3]);
  const char *mode = argv[4];
  std::vector<int> lens;
  for (char *tok = strtok(argv[5], ","); tok; tok = strtok(nullptr, ",")) lens.push_back(atoi(tok));
  const int n = (int)lens.size();
  if (hidden + 1 > width) return 2;
  std::vector<float> in((size_t)n * width), sep((size_t)n * width, -7777.0f), fallback((size_t)width);
  for (int k = 0; k < n; k++)
    for (int i = 0; i < width; i++) in[(size_t)k * width + i] = 1000.0f * k + i;
  for (int i = 0; i < width; i++) fallback[i] = -1.0f - i;
  const bool null_in = !strcmp(mode, "null"), in_place = !strcmp(mode, "inplace");
  const float *h_in = null_in ? nullptr : in.data();
  float *h_out = in_place ? in.data() : sep.data();
  TextsPlan plan;
  if (texts_plan_make(&plan, lens.data(), nullptr, n, wave_width)) return 1;
  for (int w = 0; w < plan.n_waves; w++) {
    const int rows = plan.waves[w].nrows;
    std::vector<float> staging((size_t)rows * width, -7777.0f); /* exactly the wave's rows: a row too many is out of bounds */
    texts_states_pack(&plan, w, h_in, fallback.data(), width, hidden, staging.data());
    fwrite(staging.data(), sizeof(float), staging.size(), stdout);
    for (int j = 0; j < rows; j++)
      for (int i = 1; i <= hidden; i++) staging[(size_t)j * width + i] += 0.5f;
    texts_states_unpack(&plan, w, staging.data(), width, h_out);
  }
  texts_states_fill_rowless(lens.data(), n, h_in, fallback.data(), width, hidden, h_out);
  texts_plan_free(&plan);
  fwrite(h_out, sizeof(float), (size_t)n * width, stdout);
  if (!null_in) fwrite(in.data(), sizeof(float), in.size(), stdout);
  return 0;
}
