// TEST INFRASTRUCTURE ONLY: the IoU / DIoU / CIoU box losses of
// ld_amd/csrc/ld_math.h compiled for the host with g++ (the same scalar code the
// gfx950 row kernels and the fused loss block call), so the CPU test-suite can
// check them against tests/golden/iou_losses.npz without a GPU.  The product
// never links or loads this.
#include "../ld_amd/csrc/ld_math.h"

namespace {
// mode: 0 IoU (log), 1 IoU (linear), 2 DIoU, 3 CIoU
float one(int mode, const float* p, const float* t, float eps, float* iou, float* g) {
  const ld::Box pb{p[0], p[1], p[2], p[3]}, tb{t[0], t[1], t[2], t[3]};
  switch (mode) {
    case 0: return ld::iou_loss_grad(pb, tb, eps, false, iou, g);
    case 1: return ld::iou_loss_grad(pb, tb, eps, true, iou, g);
    case 2: return ld::diou_loss_grad(pb, tb, eps, iou, g);
    default: return ld::ciou_loss_grad(pb, tb, eps, iou, g);
  }
}
}  // namespace

extern "C" {
// pred / target / grad: (rows, 4); loss / iou: (rows)
void h_box_loss_rows(int mode, const float* pred, const float* target, int rows,
                     float eps, float* loss, float* iou, float* grad) {
  for (int r = 0; r < rows; ++r)
    loss[r] = one(mode, pred + 4 * r, target + 4 * r, eps, iou + r, grad + 4 * r);
}
}
