// Stand-alone driver of Stager::copy_out (pe_stage.hpp), the threaded copy out
// of a staging buffer that the device graph build's read-back uses; built with
// -fsanitize=address,undefined by tests/test_graph_build_host.py.  No device
// call is made: the lengths around the per-thread and thread-count edges are
// copied into an exactly sized destination and compared.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pe_stage.hpp"

int main() {
    const size_t MB = (size_t)1 << 20;
    const size_t lens[] = {0, 1, 4095, 4 * MB - 1, 4 * MB, 8 * MB - 1, 8 * MB, 8 * MB + 1, 12 * MB + 13,
                           32 * MB, 32 * MB + 7, 37 * MB + 3, 64 * MB};
    std::vector<char> src(64 * MB);
    uint64_t x = 88172645463325252ull;
    for (size_t i = 0; i < src.size(); i += 8) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        std::memcpy(&src[i], &x, 8);
    }
    int fails = 0;
    for (size_t len : lens) {
        std::vector<char> dst(len);                       // exactly sized: an overrun is ASan's to find
        shdpe::Stager::copy_out(dst.data(), src.data(), len);
        if (len && std::memcmp(dst.data(), src.data(), len) != 0) {
            std::fprintf(stderr, "FAIL copy_out len %zu\n", len);
            ++fails;
        }
    }
    std::printf("stage_copy: %d failures\n", fails);
    return fails ? 1 : 0;
}
