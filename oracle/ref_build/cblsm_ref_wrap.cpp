// C entry points around the live functions of the REFERENCE's own CBLSM/CBLSM.h, compiled
// unmodified from where it lies against the container-only stand-in
// oracle/ref_build/shim/opencv2/opencv.hpp -- see oracle/Makefile.  This wrapper contains no
// algorithm: it calls the reference's functions as CBLSM.cpp does and copies nothing but what
// they wrote.  The functions of CBLSM.h that need OpenCV arithmetic (listed in the stand-in's
// header) are not reachable from here.  Test infrastructure.
#include "CBLSM.h"

#define REF_API extern "C" __attribute__((visibility("default")))

// CBLSM.cpp:64-67.  dir 0 left, 1 right, 2 up, 3 down; `tao` is passed by value as there.
REF_API int ref_cblsm_arm(unsigned char* img, int row, int col, int channels, int dir, int tao,
                          int maxLength, int secLength, int* arm)
{
    Mat image(row, col, channels, img);
    switch (dir) {
    case 0: ArmLengthL(image, uchar(tao), arm, maxLength, secLength); break;
    case 1: ArmLengthR(image, uchar(tao), arm, maxLength, secLength); break;
    case 2: ArmLengthUp(image, uchar(tao), arm, maxLength, secLength); break;
    default: ArmLengthDown(image, uchar(tao), arm, maxLength, secLength); break;
    }
    return 0;
}

REF_API int ref_cblsm_ad(unsigned char* left, unsigned char* right, int row, int col, int dispRange, int view,
                         float* vol)
{
    if (view == 0) ComputeAD(col, row, dispRange, left, right, vol);
    else ComputeADRight(col, row, dispRange, left, right, vol);
    return 0;
}

REF_API int ref_cblsm_aggregate_v5(float* vol, float* out, int* armL, int* armR, int* armUp, int* armDown,
                                   int dispRange, int row, int col)
{
    costAggregationV5(vol, out, armL, armR, armUp, armDown, dispRange, row, col, 0);
    return 0;
}

REF_API int ref_cblsm_disp(float* cost, float* disp, int dispRange, int row, int col)
{
    ComputeDispOringin(cost, disp, dispRange, row, col);
    return 0;
}

// The reference's own argument lists (CBLSM.h:65, :104, :151, :195).
REF_API int ref_cblsm_choose_lr(int dir, int* ArmLL, int* ArmLR, int* ArmRL, int* ArmRR, int dispRange,
                                int* vol, int row, int col)
{
    if (dir == 0) chooseArmLengthLeft(ArmLL, ArmLR, ArmRL, ArmRR, dispRange, vol, row, col);
    else chooseArmLengthRight(ArmLL, ArmLR, ArmRL, ArmRR, dispRange, vol, row, col);
    return 0;
}

REF_API int ref_cblsm_choose_ud(int dir, int* ArmLUp, int* ArmLDown, int* ArmRUp, int* ArmRDown, int* ArmRL,
                                int* ArmRR, int dispRange, int* vol, int row, int col)
{
    if (dir == 2) chooseArmLengthUp(ArmLUp, ArmLDown, ArmRUp, ArmRDown, ArmRL, ArmRR, dispRange, vol, row, col);
    else chooseArmLengthDown(ArmLUp, ArmLDown, ArmRUp, ArmRDown, ArmRL, ArmRR, dispRange, vol, row, col);
    return 0;
}
