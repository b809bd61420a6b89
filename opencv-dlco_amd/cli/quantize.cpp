// quantize — a float descriptor table as bytes, over libdlco.so's host calls: no GPU is needed.
//
//     quantize desc_file -out dst (-fit sample_desc_file | -quant quant_file)
//
// desc_file holds "Descriptor" [n, r] f32 (what `describe` writes).  Writes
//     "DescriptorU8" [n, r] u8     what `match -u8` reads
//     "QuantScale" [1] f32 and "QuantOffset" [r] f32     the quantiser, so that further tables can be made comparable
// -fit fits the quantiser on the "Descriptor" of sample_desc_file, which may be desc_file itself (dlco_desc_quant_fit);
// -quant reuses the two datasets of an earlier output of this tool or of `describe -quant`, bit for bit.  The rule is the
// library's own (csrc/quant_rules.hpp), not OpenCV's.  The reference has no such tool.  A path that does not end in
// .h5/.hdf5 is a directory of .npy files with the same dataset names (dlco_io.hpp).
#include "../../include/dlco.h"
#include "quant_io.hpp"

#include <cstdlib>
#include <cstring>
#include <iostream>

using std::cout;
using std::endl;

int main(int argc, char **argv)
{
    bool help = false;
    const char *src = nullptr, *out = nullptr, *fit = nullptr, *quant = nullptr;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-fit") == 0 && has_val) { fit = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-quant") == 0 && has_val) { quant = argv[++i]; continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!src) { src = argv[i]; continue; }
            help = true;
        }
    }
    if (!src || !out) help = true;
    if ((fit != nullptr) == (quant != nullptr)) {
        if (src && out) cout << "ERROR: give one of -fit and -quant." << endl;
        help = true;
    }
    if (help) {
        cout << endl;
        cout << "Usage: quantize desc_file -out dst_h5_filename (-fit sample_desc_file | -quant quant_file)" << endl;
        cout << endl;
        return 1;
    }
    try {
        std::vector<size_t> shape, sshape;
        std::vector<float> Y, S, offset;
        float scale = 0.f;
        dlco_io::read_dataset<float>(src, "Descriptor", shape, Y);
        if (shape.size() != 2 || shape[0] < 1 || shape[1] < 1 || shape[1] > 1024)
            throw std::runtime_error(std::string(src) + ": Descriptor must be a non-empty [n, r] table with r <= 1024");
        const size_t n = shape[0], r = shape[1];
        if (fit) {
            dlco_io::read_dataset<float>(fit, "Descriptor", sshape, S);
            if (sshape.size() != 2 || sshape[0] < 1 || sshape[1] != r)
                throw std::runtime_error(std::string(fit) + ": the sample must be a non-empty [n, " + std::to_string(r) + "] Descriptor table");
            offset.resize(r);
            if (dlco_desc_quant_fit(S.data(), (int64_t)sshape[0], (int32_t)r, &scale, offset.data()) != DLCO_OK)
                throw std::runtime_error(std::string(fit) + ": Descriptor contains NaN or infinity, no quantiser fits");
        } else {
            quant_io::read(quant, r, scale, offset);
        }
        std::vector<uint8_t> U(n * r);
        if (dlco_desc_quantize(Y.data(), (int64_t)n, (int32_t)r, scale, offset.data(), U.data()) != DLCO_OK)
            throw std::runtime_error("the quantiser is not valid (scale " + std::to_string(scale) + ")");
        {
            dlco_io::Writer wr(out);
            wr.write<uint8_t>("DescriptorU8", U.data(), n, r);
            quant_io::write(wr, scale, offset);
        }
        printf("Descriptors: %zu x %zu, scale %.9g\n", n, r, (double)scale);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "quantize: %s\n", e.what());
        return 2;
    }
    return 0;
}
