// tfl_reader_check - the TFLite reader (csrc/tflite_model.h) alone, for a host sanitizer: parses every file named on the command
// line, whole and truncated at EVERY byte offset, each time from a heap copy of exactly that size (so a read past the end is a
// heap overflow the sanitizer sees, not a read of the next bytes of the file). CPU only: no HIP, no device.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I tiny-object-detection_amd/csrc \
//       tools/tfl_reader_check.cpp -o /tmp/tfl_reader_check
//   python tools/tfl_reader_models.py /tmp/models && /tmp/tfl_reader_check /tmp/models/*.tflite
//
// Prints one line per file - the whole file's verdict and how many truncations parsed / were refused - and exits 0; a sanitizer
// report ends it non-zero.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "tflite_model.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        const std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (file.empty()) { fprintf(stderr, "%s: cannot read\n", argv[a]); return 2; }
        size_t ok = 0, refused = 0;
        std::string whole;
        for (size_t n = 0; n <= file.size(); ++n) {
            uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
            memcpy(copy, file.data(), n);
            yh::TflModel m;
            const bool good = m.parse(copy, n);
            (good ? ok : refused)++;
            if (n == file.size()) whole = good ? "ok, " + std::to_string(m.tensors.size()) + " tensors, " + std::to_string(m.ops.size()) + " operators" : "refused: " + m.error;
            free(copy);
        }
        printf("%s: %s; of %zu truncations %zu parsed, %zu refused\n", argv[a], whole.c_str(), file.size(), ok - (whole.rfind("ok", 0) == 0), refused);
    }
    return 0;
}
