// fb_batch_lds_bytes (simgrid_amd/csrc/lmm_fb_batch_kernels.hpp) on the host: prints the LDS bytes of a workgroup,
// without and with the weights, for every "nv nc nnz" triple of the command line (tests/test_fb_batch.py).
#include <cstdio>
#include <cstdlib>

#include "lmm_fb_batch_kernels.hpp"

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) {
    std::fprintf(stderr, "usage: %s nv nc nnz [nv nc nnz ...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 2 < argc; i += 3) {
    const int nv = std::atoi(argv[i]), nc = std::atoi(argv[i + 1]), nnz = std::atoi(argv[i + 2]);
    const size_t b = lmmdev::fb_batch_lds_bytes(nv, nc, nnz);
    std::printf("%zu %zu\n", b, b + lmmdev::fb_batch_lds_weights(nnz));
  }
  return 0;
}
