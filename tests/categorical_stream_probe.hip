// Host probe of put_network_wide (csrc/nig_mlp_stream.hpp) for tests/test_categorical_host.py: the image and the tail of the
// network IN -> 256 -> 256 -> OUT, built by the library's own builder on this machine's CPU.
//   categorical_stream_probe IN OUT weights.bin image.bin tail.bin
// weights.bin: W1 [IN][256], b1, W2 [256][256], b2, W3 [256][OUT], b3 as float32, back to back.  Prints "ok floats tail_floats".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nig_mlp_stream.hpp"

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const int IN = atoi(argv[1]), OUT = atoi(argv[2]), H = nig::MLP_H;
    const size_t nw = (size_t)IN * H + H + (size_t)H * H + H + (size_t)H * OUT + OUT;
    std::vector<float> w(nw);
    FILE *f = fopen(argv[3], "rb");
    if (!f || fread(w.data(), sizeof(float), nw, f) != nw) return 3;
    fclose(f);
    const float *W1 = w.data(), *b1 = W1 + (size_t)IN * H, *W2 = b1 + H, *b2 = W2 + (size_t)H * H, *W3 = b2 + H, *b3 = W3 + (size_t)H * OUT;
    std::vector<float> image(nig::MLP_CSTREAM_FLOATS, 0.0f), tail(nig::MLP_TAIL_FLOATS, 0.0f);
    const bool ok = nig::put_network_wide(IN, OUT, W1, b1, W2, b2, W3, b3, image.data(), image.size(), tail.data());
    f = fopen(argv[4], "wb");
    if (!f || fwrite(image.data(), sizeof(float), image.size(), f) != image.size()) return 4;
    fclose(f);
    f = fopen(argv[5], "wb");
    if (!f || fwrite(tail.data(), sizeof(float), tail.size(), f) != tail.size()) return 4;
    fclose(f);
    printf("%d %zu %zu\n", ok ? 1 : 0, image.size(), tail.size());
    return 0;
}
