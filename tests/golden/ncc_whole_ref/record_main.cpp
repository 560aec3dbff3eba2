// The recording program of tests/golden/make_ncc_whole_golden.py: calls the reference's ncc() and bgr_to_grey()
// (NCC/NCC.h, found through -I, compiled unmodified) on raw bytes from stdin and writes the result's bytes to stdout.
//   record_main left|right H W   < L bytes then R bytes      > depth bytes
//   record_main grey H W         < B, G, R interleaved       > grey bytes
// Our own text; the container behind it is ncc_whole_ref/opencv2/opencv.hpp.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "NCC.h"

static void slurp(unsigned char *dst, size_t n)
{
    if (fread(dst, 1, n, stdin) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const int H = atoi(argv[2]), W = atoi(argv[3]);
    const size_t n = (size_t)H * W;
    if (!strcmp(argv[1], "grey")) {
        Mat bgr(H, W, CV_8UC3);
        slurp(bgr.bytes(), 3 * n);
        Mat grey = bgr_to_grey(bgr);
        fwrite(grey.bytes(), 1, n, stdout);
        return 0;
    }
    Mat in1(H, W, CV_8UC1), in2(H, W, CV_8UC1);
    slurp(in1.bytes(), n);
    slurp(in2.bytes(), n);
    Mat depth = ncc(in1, in2, argv[1]);
    if (depth.rows != H || depth.cols != W) return 3;
    fwrite(depth.bytes(), 1, n, stdout);
    return 0;
}
