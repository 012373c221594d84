// decoder_choice_san.hip — the decoder-kernel resolver (pv_sdec_fused_bf16.hip: pv_sdec_fused_choice) and its launch-free consumers
// under the host sanitizers: a stand-alone program, CPU only, nothing is launched and no device is needed.
//
//   cd pyroved_amd/csrc && make all experiments      (the other sources' objects: what the selection source calls into)
//   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -Xarch_host -g"
//   H="hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -I."          (the sanitizers instrument the host pass alone)
//   $H $SAN -c ../../scripts/decoder_choice_san.hip -o /tmp/san_main.o
//   $H $SAN -mllvm --amdgpu-sched-strategy=iterative-ilp [-DPV_EXPERIMENTS] -c pv_sdec_fused_bf16.hip -o /tmp/san_sel.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/san_main.o /tmp/san_sel.o \
//         $(ls *.o | grep -v pv_sdec_fused_bf16.o) -o /tmp/decoder_choice_san          (exp/*.o with -DPV_EXPERIMENTS)
//   /tmp/decoder_choice_san        prints the number of choices resolved and a checksum; a finding aborts.  The experiments build
//                                  also under its switches: PV_W8=1 PV_X3_KERNEL=w231 /tmp/decoder_choice_san
//
// Walks the grid of tests/_decoder_choice_cases.py (fused x units x grads x sel) through the resolver, the test hook, the weight
// images' arguments and the three name hooks.
#include "pv_sdec_fused.h"
#include "pv_fb_layout.h"
#include <stdio.h>
#include <string.h>

extern "C" int pv_debug_decoder_choice(int fused, int64_t units, int grads, int sel, int64_t* out);
extern "C" const char* pv_debug_decoder_kernel_name(int fused, int64_t units, int grads, int lik);
extern "C" const char* pv_debug_decoder_kernel_name_fold(int grads, int lik);

int main() {
  const int fused[] = {0, 1, 2, 3};
  const int64_t units[] = {1, 255, 256, 1023, 1024, 1535, 1536, 1537, 32767, 32768, (1ll << 26) - 1, 1ll << 26, 1ll << 27};
  const int sels[] = {0, 1, 2, 21, 28, 4, 8, 23, 31, 33, 26, 27, 29, 41, 48, 3, 5, 99, -1};
  unsigned long long sum = 0;
  long n = 0;
  for (int f : fused)
    for (int64_t u : units)
      for (int g = 0; g < 2; ++g) {
        for (int sel : sels) {
          const PvDecChoice c = pv_sdec_fused_choice(f, u, g != 0, sel);
          int64_t out[14];
          if (pv_debug_decoder_choice(f, u, g, sel, out) != 0) return 1;
          if (out[1] != c.family || out[5] != c.waves || out[6] != c.rec_fmt || out[8] != c.park_bytes(pv_sdec_fused_grid(u))) return 2;
          PvFused pf{};
          pf.units = u; pf.sel = sel; pf.B = 7; pf.kmax = 3 * c.waves;
          const PvFbPrep p = pv_sdec_fused_bf16_prep_args(pf, g != 0, c);
          if (p.mode != c.img_mode || p.scale != c.img_scale || p.qswap != c.img_qswap) return 3;
          for (int i = 0; i < 14; ++i) sum = sum * 1000003ull + (unsigned long long)out[i];
          sum += (unsigned long long)p.nzero4;
          ++n;
        }
        for (int lik = 0; lik < 4; ++lik) {
          sum += strlen(pv_debug_decoder_kernel_name(f, u, g, lik)) + strlen(pv_debug_decoder_kernel_name_fold(g, lik)) +
                 strlen(pv_sdec_fused_bf16_wt_kernel_name(f == 2, g, lik));
        }
      }
  printf("%ld choices resolved, checksum %llx\n", n, sum);
  return 0;
}
