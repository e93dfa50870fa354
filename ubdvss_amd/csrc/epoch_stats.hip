// Epoch logs on the device for gfx950: the loss vector of a step -> the size-weighted sums that Keras' BaseLogger keeps per epoch
// (fit_generator of train.py:176-188: logs[k] = sum(value_k * batch_size) / seen; evaluate_generator averages the val_ values the
// same way).  The train loop adds every step's vector to a device accumulator on the step's own stream and reads the accumulator
// ONCE per epoch, so no step waits for the host.  No handle, no host synchronisation, no allocation; capturable in a HIP graph.
//
// Values, in accumulator order (ubdvss_amd/keras_metrics.py metrics_from_loss_vector is the single definition; this restates it
// in double from the fp32 entries of the vector, operation for operation -- the unit is built with -ffp-contract=off so that
// acc + value * n rounds the product and the sum separately, as the host restatement does):
//    0 loss                       total
//    1 detection_pixel_acc        (tp + tn) / max(1, n_pix)
//    2 detection_pixel_precision  tp / max(1, tp + fp)
//    3 detection_pixel_recall     tp / max(1, tp + fn)
//    4 detection_pixel_f1         ((2 p) r) / (p + r), 0 when p + r == 0
//    5 classification_pixel_acc   cls_ok / max(1, n_pos)
//    6 positive_loss   7 negative_loss   8 hard_negative_loss   9 detection_loss   10 classification_loss
// acc[0] += n_images (Keras' `seen`), acc[1] += 1 when the total is not finite, acc[2 + i] += value_i * n_images.  A value that
// is not finite goes into its sum as it would in BaseLogger; acc[1] lets the host say so.
//
// One launch of one wave: lane i owns slot i, so there is nothing to reduce and no atomic; launches on one stream are ordered.
#include "common.h"

#define ES_VALUES UBD_EPOCH_VALUES
#define ES_SLOTS (2 + ES_VALUES)

// Python's max(1.0, x): x only when it is greater
__device__ __forceinline__ double es_max1(double x) { return x > 1.0 ? x : 1.0; }

__global__ __launch_bounds__(64) void es_accumulate_kernel(const float *__restrict__ loss, int n_images, double *__restrict__ acc)
{
    const int slot = threadIdx.x;
    if (slot >= ES_SLOTS) return;
    const double total = loss[0], det = loss[1], cls = loss[2];
    const double pos_l = loss[4], neg_l = loss[5], hard_l = loss[6], n_pos = loss[7];
    const double tp = loss[8], tn = loss[9], fp = loss[10], fn = loss[11], cls_ok = loss[12], n_pix = loss[13];
    const double n = (double)n_images;
    if (slot == 0) { acc[0] = acc[0] + n; return; }
    if (slot == 1) {
        if (!(fabs(total) <= 1.7976931348623157e308)) acc[1] = acc[1] + 1.0;      // NaN or an infinity
        return;
    }
    const double precision = tp / es_max1(tp + fp);
    const double recall = tp / es_max1(tp + fn);
    double v;
    switch (slot - 2) {
    case 0: v = total; break;
    case 1: v = (tp + tn) / es_max1(n_pix); break;
    case 2: v = precision; break;
    case 3: v = recall; break;
    case 4: v = (precision + recall != 0.0) ? ((2.0 * precision) * recall) / (precision + recall) : 0.0; break;
    case 5: v = cls_ok / es_max1(n_pos); break;
    case 6: v = pos_l; break;
    case 7: v = neg_l; break;
    case 8: v = hard_l; break;
    case 9: v = det; break;
    default: v = cls; break;
    }
    const double weighted = v * n;
    acc[slot] = acc[slot] + weighted;
}

extern "C" size_t ubd_epoch_accumulator_bytes(void) { return (size_t)ES_SLOTS * sizeof(double); }

extern "C" int ubd_epoch_accumulate(const float *loss, int n_images, double *acc, void *stream)
{
    UBD_REQUIRE(loss && acc, "ubd_epoch_accumulate: null argument");
    UBD_REQUIRE(n_images >= 1, "ubd_epoch_accumulate: n_images must be >= 1, got %d", n_images);
    UBD_REQUIRE(((uintptr_t)acc & 7) == 0 && ((uintptr_t)loss & 3) == 0, "ubd_epoch_accumulate: misaligned argument");
    hipLaunchKernelGGL(es_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, n_images, acc);
    UBD_CHECK_HIP(hipGetLastError());
    return 0;
}
