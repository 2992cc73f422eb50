// deflate_writer_main.cpp -- TEST INFRASTRUCTURE.  One stream of every flush
// kind, params(), tune(), prime() and reset() through
// deflate_writer_backend.cpp, for a sanitizer run on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       deflate_writer_main.cpp deflate_writer_backend.cpp -o dw_asan && ./dw_asan
#include <cstdio>
#include <vector>

#include "../../include/beast_pmd.h"

int main()
{
    const int flushes[] = {BPMD_FLUSH_SYNC,  BPMD_FLUSH_NONE, BPMD_FLUSH_PARTIAL, BPMD_FLUSH_BLOCK, BPMD_FLUSH_FULL,
                           BPMD_FLUSH_TREES, BPMD_FLUSH_NONE, BPMD_FLUSH_BLOCK,   BPMD_FLUSH_FINISH};
    std::vector<unsigned char> in(70000), out(7);   // two stored blocks a flush, handed out 7 bytes a call
    for (size_t i = 0; i < in.size(); ++i) in[i] = (unsigned char)(i * 131 >> 3);
    bpmd_stream* s = nullptr;
    if (bpmd_deflate_stream_create(6, 15, 8, 0, &s) != 0) return 1;
    size_t total = 0;
    for (int round = 0; round < 2; ++round) {
        bpmd_zparams zs{};
        int r = bpmd_deflate_stream_prime(s, 10, 2);
        for (int f : flushes) {
            zs.next_in = in.data();
            zs.avail_in = in.size() - (size_t)f * 9000;
            do {
                zs.next_out = out.data();
                zs.avail_out = out.size();
                r = bpmd_deflate_stream_write(s, &zs, f);
            } while (r == BPMD_OK && zs.avail_out == 0);
            if (r < 0 || r == BPMD_STREAM_ERROR) return 2;
            if (f == BPMD_FLUSH_PARTIAL) r = bpmd_deflate_stream_tune(s, 4, 4, 8, 4);
            zs.next_out = out.data();
            zs.avail_out = out.size();
            if (f == BPMD_FLUSH_NONE && bpmd_deflate_stream_params(s, &zs, 1 + round, 2) < 0) return 3;
        }
        if (r != BPMD_END_OF_STREAM) return 4;
        total += zs.total_out;
        bpmd_deflate_stream_reset(s);
    }
    bpmd_stream_destroy(s);
    std::printf("ok: %zu bytes out\n", total);
    return 0;
}
