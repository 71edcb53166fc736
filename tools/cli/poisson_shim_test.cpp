// poisson_shim_test.cpp -- fft_gpu::tvDeblurPoisson_RGB on three raw float32 planes, for tests/test_tvpoisson_gpu.py::test_cpp_wrapper to
// compare with the C call the wrapper is defined by.
// usage: poisson_shim_test <in.f32: 3 planes> <rows> <cols> <psf-size> <psf-angle> <mu> <iterations> <rho> <background> <coupled 0|1> <out.f32>
#include "utils.hpp"
#include "fft/fft.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
    if (argc < 12) {
        std::printf("usage: poisson_shim_test <in.f32> <rows> <cols> <psf-size> <psf-angle> <mu> <iterations> <rho> <background> <coupled 0|1> <out.f32>\n");
        return -1;
    }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), size = std::atoi(argv[4]);
    if (rows <= 0 || cols <= 0 || size <= 0) return -1;
    std::vector<Mat> ch;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (int k = 0; k < 3; ++k) {
        Mat m(rows, cols, CV_32F);
        if (std::fread(m.ptr<float>(0), sizeof(float), (size_t)rows * cols, f) != (size_t)rows * cols) { std::fprintf(stderr, "short read\n"); return 2; }
        ch.push_back(m);
    }
    std::fclose(f);
    Mat psf(size, size, CV_32F);
    if (fdr_psf_motion(size, std::atof(argv[5]), psf.ptr<float>(0)) != FDR_OK) { std::fprintf(stderr, "%s\n", fdr_last_error()); return 3; }
    fft_gpu::tvDeblurPoisson_RGB(ch, psf, std::strtof(argv[6], nullptr), std::atoi(argv[7]), std::strtof(argv[8], nullptr), Mat(),
                                 std::strtof(argv[9], nullptr), std::atoi(argv[10]) != 0);
    f = std::fopen(argv[11], "wb");
    if (!f) return 2;
    for (const Mat& m : ch) std::fwrite(m.ptr<float>(0), sizeof(float), (size_t)rows * cols, f);
    std::fclose(f);
    return 0;
}
