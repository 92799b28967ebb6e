// tflite_exec.h — what the TFLite executor's two units share: the kernels' parameter structs and one launcher per kernel family
// (tflite_kernels.hip: the device code; tflite_exec.hip: the plan and the C ABI). Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// (hidden: nothing declared here is exported from the shared library)
namespace yh __attribute__((visibility("hidden"))) {

// Operators folded into their producer at plan time (round 4, yh_tuning.tfl_fuse): the producer computes its own uint8 output
// value exactly as TFLite does - in a register - and the element-wise operators that consumed it (QUANTIZE / RELU / RELU6 as a
// requantisation, TANH as its 256-entry table, ADD with its other operand read from memory) run on that value before the one
// store: the same integers in the same order, no intermediate tensor, no launch. A CONCATENATION part with the output's own
// quantisation is written by its producer straight into the concatenated tensor, a PAD in front of a convolution becomes that
// convolution's padding (a padded tap holds the zero point: (x - zx) = 0, the tap TFLite's kernels skip).
// int8 tensors (DESIGN.md section 11 "TFLite int8"): the value in the register is the true integer whatever the tensor's type, so a
// requantisation step is the same code with the output type's range in lo / hi and a folded chain may change type; signedness
// matters only where memory is read - the ADD's other operand (a template parameter of apply_post: the producer's own signedness,
// fuse_plan folds no ADD of another type), the table's index (a signed input's table has 384 entries, index -128 .. 255, and
// `lut` points at index 0: the true integer and the raw byte find the same entry) and the table's entry (step kind 4 reads it as int8).
struct PostStep { int kind; int zi, zo, m, s, lo, hi; const uint8_t* lut; };   // 1 requantise, 2 table, 3 the ADD below, 4 int8 table
struct PostOps {
    int n;
    PostStep st[3];
    const uint8_t* other; long long other_s;    // ADD: the other operand (same shape), bytes per image
    int q_is_a, za, zb, m1, s1, m2, s2, mo, so, azo, alo, ahi;
};

// A convolution: the host's one record of it (tflite_exec.hip: Prepared) and the argument of every kernel but the int8 MFMA ones
struct ConvQ {
    const uint8_t *x, *w; const int* bias; uint8_t* y;
    int H, W, Ci, Ho, Wo, Co, kh, kw, sh, sw, ph, pw, dh, dw, dm;
    int zx, zw, zo, mult, shift, lo, hi;
    const int* wsum;   // [Co][kh*kw]: sum of the raw weight bytes of one tap (dot-product kernel), or nullptr
    // batch plan (yh_tfl_set_batch): the grid's last used dimension is the image; activations are image-major
    long long xs, ys;  // bytes per image of x / y
    PostOps po;
    // int8 activations, symmetric int8 weights (zw = 0): one multiplier and shift per output channel, [Co] padded to 64s (a weight
    // tensor with a single scale: all equal), and the kernels' signed forms (sgn: the launcher's choice, nothing a kernel reads)
    const int *mtab, *stab;
    int sgn;
};
// The argument of the int8 MFMA kernels, built from the record for one image count when a launch or a group is made (conv_i8_args)
struct ConvI8 {
    const uint8_t* x; const uint8_t* wq; const int* cterm; uint8_t* y;   // wq: [CoPad][K] bytes w ^ 0x80, K = (r, s, c); cterm: [CoPad]
    int H, W, Ci, Ho, Wo, Co, kh, kw, sh, sw, ph, pw, dh, dw;
    int zx, zw, zo, mult, shift, lo, hi, K, M;
    long long xs, ys;
    PostOps po;
    // int8 (sgn): wq holds the weight bytes as they are (padding rows 0), cterm[oc] = bias[oc] - zx sum_k w[oc, k], and the epilogue
    // takes channel oc's multiplier and shift from mtab / stab [CoPad]
    const int *mtab, *stab;
    int sgn;
};
struct AddQ { const uint8_t *a, *b; uint8_t* y; long long n; int za, zb, zo, m1, s1, m2, s2, mo, so, lo, hi; int sgn; };   // sgn: int8 operands and output
struct PadQ { const uint8_t* x; uint8_t* y; int id[4], od[4], before[4]; int fill; };
struct ResizeQ {
    const uint8_t* x; uint8_t* y; int H, W, C, Ho, Wo; float hs, ws; int half_pixel; long long ys; PostOps po;
    int sgn, hs10, ws10;   // int8: TFLite's integer kernel, the two steps in 10-bit fixed point
};
// copy one concat input [outer][inner] into the output at column `off` of rows of `row` elements
struct CatQ { const uint8_t* x; uint8_t* y; long long outer; int inner, row, off, esz; int rescale; float sc, bias; int zo; };

constexpr int kPx8MaxK = 512;   // taps x input channels a launch of tfl_conv_u8_px8 can hold (16 KB of LDS)
constexpr int kMaxGroup = 16;   // convolutions of one tfl_conv_i8_direct_group launch

// One launcher per kernel family. `nb` = the images of this invoke: the per-image structs are launched over nb images (a grid
// dimension, or nb x the elements of an image-major activation); a ConvI8 holds its image count in M. Launch errors are left to
// the caller's hipGetLastError().
// CONV_2D: the dot-product kernel where p.wsum is set, else (dot) the 8-channels-per-lane kernel while its weights fit LDS, else one lane per element
enum ConvU8Kernel { CONV_U8_SCALAR, CONV_U8_PX8, CONV_U8_DOT1, CONV_U8_DOT4 };
ConvU8Kernel conv_u8_kernel(const ConvQ& p, bool dot);   // the kernel launch_conv_u8 runs (also what yh_tfl_op_info reports)
void launch_conv_u8(const ConvQ& p, bool dot, unsigned nb, hipStream_t s);
// DEPTHWISE_CONV_2D: (dot) four channels per lane where the layer allows it, else one lane per element
bool dwconv_u8_takes_c4(const ConvQ& p, bool dot);       // the choice launch_dwconv_u8 makes (also what yh_tfl_op_info reports)
void launch_dwconv_u8(const ConvQ& p, bool dot, unsigned nb, hipStream_t s);
void launch_conv_i8_mfma(const ConvI8& q, hipStream_t s);
// The register-fed int8 kernel is built in a table of forms (ring depth, whole K in one pass, compile-time extent).
int conv_i8_direct_form(int kh, int kw, int Ci);   // the table row a convolution runs, < 0: the table has none for it
int conv_i8_direct_form_count();                   // the table's rows, and row i's (D, ONCE, KK) (yh_tfl_direct_forms)
void conv_i8_direct_form_row(int i, int* D, int* once, int* KK);
bool conv_i8_direct_pays(const ConvI8& q);         // this launch is faster register-fed than on the LDS tiles
void launch_conv_i8_direct(int form, const ConvI8& q, hipStream_t s);
// ... several convolutions of one form as one launch: parameter blocks and tile prefix table in device memory, `tiles` workgroups
void launch_conv_i8_direct_group(int form, bool sgn, const ConvI8* probs, const int* tile_start, int nprob, int tiles, hipStream_t s);
void launch_add_u8(const AddQ& p, unsigned nb, hipStream_t s);
// (sgn: the input / the output / the input is int8; the requantisation's output type is in its lo / hi)
void launch_requant_u8(const uint8_t* x, uint8_t* y, long long n, int zi, int zo, int m, int sh, int lo, int hi, hipStream_t s, bool sgn = false);
void launch_quantize_f32(const float* x, uint8_t* y, long long n, float scale, int zo, hipStream_t s, bool sgn = false);
void launch_dequantize_u8(const uint8_t* x, float* y, long long n, float scale, int z, hipStream_t s, bool sgn = false);
void launch_lut_u8(const uint8_t* x, uint8_t* y, long long n, const uint8_t* lut, hipStream_t s);
void launch_pad_u8(const PadQ& p, unsigned nb, hipStream_t s);
void launch_resize_bilinear_u8(const ResizeQ& p, unsigned nb, hipStream_t s);
void launch_concat_part(const CatQ& p, unsigned nb, hipStream_t s);
void launch_copy_bytes(const uint8_t* x, uint8_t* y, long long n, hipStream_t s);

}  // namespace yh
