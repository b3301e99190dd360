/*
 * include/escoin.h -- C ABI of libescoin_hip.so
 *
 * MI355X (gfx950) direct sparse convolution forward: the drop-in for the path
 *   ConvolutionLayer<Dtype>::Forward_gpu            src/caffe/layers/conv_layer.cu:8-40
 *     -> BaseConvolutionLayer::forward_gpu_sconv[_par]   base_conv_layer.cpp:748-848
 *        -> caffe_gpu_sconv + forward_gpu_bias           math_functions.cu:590-704,
 *                                                        base_conv_layer.cpp:850-856
 *   fed by BaseConvolutionLayer::WeightAlign             base_conv_layer.cpp:46-273
 * of chenxuhao/caffe-escoin (file:line relative to the reference tree).
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no torch / STL types cross this boundary;
 *   - every entry point returns 0 on success and a negative ESCOIN_E* code on
 *     failure; escoin_last_error() returns the message of the calling thread's last
 *     failure.  The reference aborts on every error (glog CHECK / CUDA_CHECK,
 *     include/caffe/util/device_alternate.hpp:51-78); the C++ Layer shim
 *     (caffe-escoin_amd/caffe_shim/) turns a non-zero return into that abort;
 *   - all tensors fp32 NCHW contiguous, all indices int32, as in the reference;
 *   - device pointers are HIP device pointers on the current device; `stream` is a
 *     hipStream_t passed as void* (NULL = the default stream, which is what every
 *     reference kernel launch uses);
 *   - the caller owns bottom / top / bias / dense-weight memory; a plan owns its CSR
 *     arrays, the blocked weight streams and its scratch, and frees them in
 *     escoin_plan_destroy (reference: layer dtor, base_conv_layer.cpp:16-42);
 *   - thread-compatible: one plan per (host thread, device), like a Caffe layer
 *     instance (common.cpp:13-19 keeps the Caffe singleton thread-local).
 *   - no SILENT CPU fallback: the GPU entry points (escoin_weight_align, escoin_forward, the escoin_gpu_* helpers)
 *     fail with ESCOIN_ENODEVICE when no HIP device is visible, they never compute on the host.  Caffe::CPU mode
 *     (ConvolutionLayer::Forward_cpu, conv_layer.cpp:25-63) is a separate, explicit set of entry points --
 *     escoin_weight_align_cpu / escoin_forward_cpu / escoin_cpu_* below -- implemented in this library
 *     (csrc/sconv_cpu*.cpp) and usable on a machine without a GPU;
 *   - Dtype: the reference instantiates the path for float and double (conv_layer.cpp:102, conv_layer.cu:75,
 *     math_functions.cu:696-704,765-766, math_functions.cpp:178-199).  Every unsuffixed entry point is the float
 *     one; the `_f64` twins take double.  A plan's type is fixed by the align call (weight_align[_cpu][_f64] /
 *     set_csr[_f64]); calling the other type's forward on it is ESCOIN_ESTATE.  north_star measures fp32: double
 *     plans run the order-preserving generic kernel on the device (fp64 vector FMA is native on gfx950) and the same
 *     host kernel as float in CPU mode -- no LDS-tiled / generated-code / MFMA fast path.
 */
#ifndef ESCOIN_H_
#define ESCOIN_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Symbol visibility: the library is built with -fvisibility=hidden. */
#if defined(ESCOIN_BUILD) && defined(__GNUC__)
#define ESCOIN_API __attribute__((visibility("default")))
#else
#define ESCOIN_API
#endif

#define ESCOIN_OK 0
#define ESCOIN_EINVAL (-1)    /* bad argument / unsupported geometry            */
#define ESCOIN_ENOMEM (-2)    /* host or device allocation failed               */
#define ESCOIN_EHIP (-3)      /* a HIP runtime call or kernel launch failed     */
#define ESCOIN_ESTATE (-4)    /* forward before weight_align / set_csr          */
#define ESCOIN_ENODEVICE (-5) /* no HIP device visible                          */

/* ---- Size limits --------------------------------------------------------------------------------------------------
 * Blobs are addressed in 64 bits wherever nothing below says otherwise; every limit is a host-side rule (csrc/align_rules.h,
 * held to its edge by tests/cpp/launch_limits_check.cpp) and every refusal is ESCOIN_EINVAL with a message, before
 * anything is launched.  Sizes of one call: n images, bottom n*C*H*W, top n*M*OH*OW floats.
 *
 *   what                                     limit                          beyond it
 *   tiled / generated code: bottom of one    0xFFFFFFF0 bytes (a buffer     the call runs as consecutive launches of
 *     launch                                 descriptor's 32-bit offsets)   (0xFFFFFFF0 - 16) / image_bytes images
 *   tiled / generated code: one image        below 0xFFFFFFF0 bytes         refused
 *   tiled / generated code: top of one       below 2^31 bytes for the asm   the launch stores element-wise from the
 *     launch                                 epilogues' 32-bit offsets      generic compiled body: same results
 *   strided pointwise (1x1, stride 2) top    below 2^31 bytes               refused
 *   tiled: conv groups x workgroup columns   65535 (grid y)                 refused
 *   dense MFMA kernel: bottom of the call,   below 0xFFFFFFF0 bytes each    refused
 *     weight matrix
 *   dense MFMA kernel: n*OH*OW               below 2^31                     refused
 *   generic kernel: n, ceil(M / 4)           65535 each (grid z, y)         refused
 *   LOWERED_SPARSE: rows, columns, images    65535 each (grid y, z)         refused
 *   Backward: N, Mg; C                       65535; 4 x 65535               refused (bwd_choice)
 *   staged weight gradient                   N*M*OH*OW, N*C*H*W < 2^31      refused when forced, AUTO takes the entry kernel
 *   MFMA weight / data gradient, dense       N*OH*OW (N*H*W), M*Cg*KH*KW,   refused when forced (wgm_plan, dgm_plan)
 *     weight gradient                        Cg*H*W (Mg*OH*OW) < 2^31
 *   options "s2d", "s2b", "b2s"              bottom, top, X', T' < 2^31     the option is not taken: the plan runs as
 *                                            elements; N*P, N' <= 65535     without it
 * A plan whose conv groups are split between the dense and the sparse kernels asks the sparse half's limits before it
 * launches the dense half: a refused call has written nothing. */

/* Caffe::ConvMode, include/caffe/common.hpp:112.  The two direct-sparse modes differ in the
 * reference only by launch granularity (per image vs whole batch, conv_layer.cu:16-26) and produce
 * the same numbers; LOWERED_GEMM is the dense MFMA kernel, LOWERED_SPARSE the lowering comparator. */
#define ESCOIN_CONV_MODE_LOWERED_GEMM 0
#define ESCOIN_CONV_MODE_LOWERED_SPARSE 1
#define ESCOIN_CONV_MODE_SCONV 2
#define ESCOIN_CONV_MODE_SCONV_PAR 3

/* Which kernel family a plan uses (escoin_plan_set_option("kernel", ...)). */
#define ESCOIN_KERNEL_AUTO 0
#define ESCOIN_KERNEL_GENERIC 1 /* one lane = one output pixel, CSR order kept    */
#define ESCOIN_KERNEL_TILED 2   /* LDS-staged tiles, row-grouped weight stream    */
#define ESCOIN_KERNEL_DENSE 3   /* implicit-GEMM on the fp32 matrix cores (MFMA)  */
#define ESCOIN_KERNEL_JIT 4     /* LDS-staged tiles; the weight walk is machine code
                                   WeightAlign generated from the sparsity pattern
                                   (what AUTO runs on every stride-1 layer -- and on
                                   1x1 / stride-2 layers -- that it keeps on the sparse
                                   path; the one exception is the small-launch rule,
                                   escoin_plan_stat "small_launch_rule")              */

/* Geometry of one ConvolutionLayer: what LayerSetUp/Reshape derive from
 * ConvolutionParameter + the bottom shape (base_conv_layer.cpp:276-530). */
typedef struct escoin_conv_desc {
  int N;        /* num_: largest batch a forward call may carry                 */
  int C, H, W;  /* channels_ (all groups), conv_input_shape_[1..2]              */
  int M;        /* num_output_ (all groups)                                     */
  int KH, KW;   /* kernel_shape_                                                */
  int pad_h, pad_w;
  int stride_h, stride_w;
  int dil_h, dil_w;
  int group;    /* group_                                                       */
  int has_bias; /* bias_term_: forward adds bias[oc] once (conv_layer.cu:21-24) */
  int fuse_relu;/* ConvolutionReLU: max(x + bias, 0) (conv_relu_layer.cu:8-30)  */
} escoin_conv_desc;

typedef struct escoin_plan escoin_plan;

/* Message of this thread's last failed call ("" if none). */
ESCOIN_API const char *escoin_last_error(void);

/* Number of visible HIP devices (0 without a GPU; never fails). */
ESCOIN_API int escoin_device_count(void);

/* ConvolutionLayer::compute_output_shape, conv_layer.cpp:8-22. */
ESCOIN_API int escoin_out_shape(const escoin_conv_desc *desc, int *out_h, int *out_w);

/* Length in elements of the reference's shared-halo padded image C(H+ph)(W+pw) + ph(W+2pw),
 * base_conv_layer.cpp:71,596 -- plus pad_w elements when pad_h == 0 < pad_w: the last row's right padding is read
 * out of the elements that follow the row, and without a bottom padding row nothing follows the last channel's last
 * row (the reference's buffer is pad_w short there and its kernels read past it; none of its models has such a
 * layer).  A zeroed buffer of this length is safe for escoin_gpu_sconv / escoin_cpu_sconv / copy_input_data. */
ESCOIN_API long escoin_padded_len(const escoin_conv_desc *desc);

/* LayerSetUp + Reshape: validates the geometry and creates an empty plan.
 * No device work happens here, so it also succeeds on a machine without a GPU. */
ESCOIN_API int escoin_plan_create(const escoin_conv_desc *desc, escoin_plan **plan);
ESCOIN_API int escoin_plan_destroy(escoin_plan *plan);

/* Options (all but "conv_mode", "cpu_channel_block", "cpu_images_per_job" and "wgrad_kernel" must precede weight_align /
 * set_csr; "wgrad_kernel" set on an aligned plan is read when the next backward state is built: by the first backward
 * after the next align, or -- when none has run on this alignment, e.g. after a refused forced kernel -- by the next one):
 *   "kernel"     = ESCOIN_KERNEL_*;
 *   "conv_mode"  = Caffe::ConvMode (common.hpp:112; tools/caffe.cpp:292-301 -conv_mode N):
 *                  SCONV / SCONV_PAR = the direct sparse path (the two differ only in the
 *                  reference's batching), LOWERED_SPARSE = the comparator (im2col + CSR x dense per
 *                  image, base_conv_layer.cpp:724-736), LOWERED_GEMM = every group on the dense
 *                  fp32-MFMA implicit-GEMM kernel (forward_gpu_gemm, base_conv_layer.cpp:713-746).
 *                  May be switched on an aligned plan;
 *   "dense_gate" = 0/1.  0 (default): KERNEL_AUTO sends EACH conv group whose own density exceeds
 *                  the measured sparse/dense crossover to the MFMA kernel and the others to the
 *                  sparse kernel.  1: reproduce the reference's gate -- density(group 0) > 0.2
 *                  sends the whole layer to the dense path (base_conv_layer.cpp:750-755,805-811);
 *   "dense_threshold_pct" = density in percent above which AUTO picks the dense kernel
 *                  (-1 = the built-in measured crossover; 100 = never);
 *   "tiling_batch" = choose the tiled kernel's tiling as for a batch of this many images
 *                  (0 = desc.N).  Results do not depend on it; tests use it to run small inputs
 *                  through the weight stream / tile shapes of the full-size configurations;
 *   "stream_stores" = 1: pointwise (1x1, stride 1, pad 0) layers write the top blob with non-temporal
 *                  stores -- for a blob nothing on the device reads next (3-4 % on a sequence of
 *                  independent layers); 0 / -1 (default): ordinary stores, which leave the blob in
 *                  L2 / Infinity Cache for the layer that consumes it (as the reference's kernels
 *                  do, math_functions.cu:524-587).  Results are the same either way;
 *   "max_launch_bytes" = bottom-blob bytes one launch of the LDS-tiled kernels may cover (0 = the 4 GiB range of
 *                  a buffer descriptor; larger batches run as consecutive sub-batch launches).  Results do not
 *                  depend on it; tests use it to exercise the sub-batch loop on small inputs.
 *   "cpu_channel_block" = input channels per block of escoin_forward_cpu's channel blocking (0 = chosen from the
 *                  geometry so that a tile's input window stays in L1; stride-1 layers only).  Results do not depend on
 *                  it (a row's sum continues across blocks in CSR order); tests use it to block small inputs.  May be set
 *                  on an aligned plan; stat "cpu_channel_block" = what the last escoin_forward_cpu used.
 *   "cpu_images_per_job" = escoin_forward_cpu runs small images (a few vectors each: 7 x 7, 4 x 4, LeNet's 8 x 8) two or three
 *                  to a job, one broadcast weight feeding every image's accumulators; 0 = chosen from the geometry,
 *                  n = at most n.  Results do not depend on it; tests use it.  May be set on an aligned plan.
 *   "code_loader" = how WeightAlign / import_aligned put generated code on the device.  0 (default): executable
 *                  device memory from the ROCm runtime's allocator, filled by a copy kernel (~0.1 ms per megabyte),
 *                  and the code object loader where that is not to be had; 1: always the code object loader
 *                  (hipModuleLoadData on the code wrapped in a code object, 0.6-1 ms per megabyte).  The code is the
 *                  same words either way; tests use 1 to exercise the fallback.  stat "code_direct" says which.
 *   "body_variant" = which compiled kernel body runs around a chained plan's generated code.  -1 (default): the
 *                  chained instantiation wherever the plan and the launch meet its conditions (csrc/align_rules.h
 *                  body_variant), the generic body otherwise; 0: always the generic body.  Both call the same code
 *                  and run the same epilogue: results are bit-identical; tests and same-call A/B runs use 0.  May be
 *                  set on an aligned plan; stat "body_variant" = what the last forward ran (0 generic, 1 chained).
 *   "code_touchers" = which workgroups of a generated-code launch pull whole lines with their code touches.  0
 *                  (default): the rule (csrc/align_rules.h touch_election: every 8th workgroup among those that share
 *                  an XCD and a grid row on a device of eight XCDs, every workgroup elsewhere); k >= 1: every k-th
 *                  (1: every workgroup; 65535 or more: the first of each set alone).  The other workgroups' touches ask
 *                  for one line instead of 64.  No instruction and no result changes; stats "code_touchers" (the
 *                  stride of the last launch) and "touch_lines_per_launch".  Not handed down to derived plans.  Stream
 *                  plans, code without touches and launches of the chained pointwise body do not elect: their
 *                  stride is 1 whatever the option says.
 *   "s2d"        = 0 (default) / 1: run a strided layer on the stride-1 kernels via space-to-depth ("Space-to-depth"
 *                  below).  1 changes nothing for a layer the option does not serve; KERNEL_AUTO never picks it by itself.
 *   "s2b"        = 0 (default) / 1: run a dilated stride-1 layer on the stride-1, dilation-1 kernels via space-to-batch
 *                  ("Space-to-batch" below).  1 changes nothing for a layer the option does not serve; KERNEL_AUTO never
 *                  picks it by itself.  May be set together with "s2d": the two serve disjoint geometries.
 *   "b2s"        = 0 (default) / 1: run an inner-product layer (H = W = 1, a 1x1 kernel, pad 0) on the pointwise kernels
 *                  with the batch as the pixel axis ("Batch-to-space" below).  1 changes nothing for a layer the option
 *                  does not serve; KERNEL_AUTO never picks it by itself.  May be set together with "s2d" and "s2b".
 *   "b2s_block"  = the block B of "b2s": 0 (default) the rule, otherwise a multiple of 4 in 4..256 (a test option).
 * Environment: the product build reads ESCOIN_VERBOSE (diagnostics on stderr) and TMPDIR (temporary file of the
 * code object manager's fallback path) and nothing else -- no environment variable can change a result
 * ("Environment"; csrc/knobs.h for the non-product flavours built by tools/mkabl.sh exp / stamps). */
ESCOIN_API int escoin_plan_set_option(escoin_plan *plan, const char *key, int value);

/* WeightAlign(): dense blobs_[0] (M x C/g x KH x KW, zeros = pruned) -> per-group CSR
 * (caffe_{cpu,gpu}_sparse_dense2csr, math_functions.cpp:77-107 / .cu:103-152), index
 * stretch (base_conv_layer.cpp:96-107 / stretch_kernel math_functions.cu:706-727) and
 * the MI355X-specific blocked weight streams; uploads everything to the device.
 * `dense_w` is a host pointer, or a device pointer when w_on_device != 0. One-time. */
ESCOIN_API int escoin_weight_align(escoin_plan *plan, const float *dense_w, int w_on_device,
                        void *stream);

/* CSR hand-off without the dense blob (what a broadcast receiver calls, the
 * counterpart of NCCL<Dtype>::Broadcast, parallel.cpp:189-200).  Host arrays:
 * rowptr[group*(M/group+1)] group-local and 0-based, colidx/values concatenated over
 * groups, colidx UNSTRETCHED (ic*KH*KW + kr*KW + kc), nnz_per_group[group]. */
ESCOIN_API int escoin_plan_set_csr(escoin_plan *plan, const int *rowptr, const int *colidx,
                        const float *values, const int *nnz_per_group, void *stream);

/* nnz of one group (nz_num_[g], base_conv_layer.cpp:247), or of all groups for
 * group < 0.  Negative on error. */
ESCOIN_API long escoin_plan_nnz(const escoin_plan *plan, int group);

/* Copies the plan's CSR to host arrays sized as in escoin_plan_set_csr.  With
 * stretched != 0 colidx is the reference's stretched index
 * (ic*(H+ph)+kr)*(W+pw)+kc, i.e. exactly nz_weight_indices_ after WeightAlign. */
ESCOIN_API int escoin_plan_get_csr(const escoin_plan *plan, int *rowptr, int *colidx, float *values,
                        int stretched);

/* Device bytes owned by the plan (CSR + weight streams / generated code + scratch, the backward state and the update state). */
ESCOIN_API size_t escoin_plan_workspace_bytes(const escoin_plan *plan);

/* The aligned form as one relocatable byte blob: the CSR and -- for a generated-code plan -- the
 * channel deal, the unit table and the machine code WeightAlign generated.  The reference recomputes
 * its aligned form on every weight load (Net::CopyTrainedLayersFrom -> WeightAlign, net.cpp:819);
 * here WeightAlign also compiles code (2-25 ms per layer since round 4, profiles/r04_weight_align.md), and a
 * deployment may persist the result once.
 *   export: buf == NULL queries the size (*bytes); otherwise writes *bytes <= capacity bytes.
 *   import: restores the CSR (always) and, when the blob's code section was written by this library
 *           build for this geometry / batch / tiling_batch, for the same split of the conv groups between the
 *           sparse and the dense kernel (options dense_threshold_pct, dense_gate, conv_mode decide it) and on a
 *           device of the same ISA and CU count, puts the persisted code on the device as it is -- no channel deal, no generator pass, no assembler, no code object loader
 *           (escoin_plan_stat(plan, "import_fast") == 1); otherwise it aligns from the CSR like
 *           escoin_plan_set_csr -- also when the persisted code cannot be placed on this device.  Plan options must be
 *           set before the import, as before weight_align.  Every field of the blob is range-checked before it
 *           sizes or indexes anything; a malformed blob gives ESCOIN_EINVAL, never a crash.  The header carries 64-bit
 *           content tags of the CSR section and of the code section and one binding the two: a blob whose code does not
 *           belong to its CSR (a torn broadcast, a spliced cache file) is refused with ESCOIN_EINVAL -- it can never
 *           run stale code on new weights.  (An integrity check against accidents, not a security boundary.) */
ESCOIN_API int escoin_plan_export_aligned(const escoin_plan *plan, void *buf, size_t capacity, size_t *bytes);
ESCOIN_API int escoin_plan_import_aligned(escoin_plan *plan, const void *buf, size_t bytes, void *stream);
/* The same from a DEVICE buffer -- where an RCCL broadcast leaves the blob (NCCL<Dtype>::Broadcast, parallel.cpp:189-200):
 * one copy into a pinned staging area the calling thread keeps between calls, then the import above. */
ESCOIN_API int escoin_plan_import_aligned_dev(escoin_plan *plan, const void *dev_buf, size_t bytes, void *stream);

/* ---- Space-to-depth: strided layers on the stride-1 kernels (option "s2d") --------------------------------------------
 * Every fast sparse kernel is a stride-1 kernel; a strided convolution is a stride-1 convolution of a rearranged input.
 * For a descriptor with dil_h = dil_w = 1 let PH = min(stride_h, KH), PW = min(stride_w, KW) (the phases that own a tap),
 * KH' = ceil(KH / stride_h), KW' = ceil(KW / stride_w), H' = OH + KH' - 1, W' = OW + KW' - 1.  The INNER plan has
 *   C' = C * PH * PW channels, c' = (c * PH + ph) * PW + pw (a conv group's channels stay contiguous: group' = group,
 *   Cg' = Cg * PH * PW), M' = M, an H' x W' image, a KH' x KW' kernel, pad 0, stride 1, dilation 1, and the outer
 *   plan's N, has_bias and fuse_relu;
 *   input   X'[n][c'][i][j] = X[n][c][i * stride_h + ph - pad_h][j * stride_w + pw - pad_w] inside the image, +0 outside;
 *   weights CSR entry (oc, c, kr, kc) -> (oc, c', kr / stride_h, kc / stride_w) with ph = kr % stride_h, pw = kc %
 *           stride_w: injective, the nonzero count and the FLOPs of the sparse walk do not change; inner positions
 *           without a preimage are never entries;
 *   top = inner_forward(X'), bias and ReLU in the inner epilogue;
 *   data gradient dX' = inner_data_gradient(top_diff), and with hp = h + pad_h, wp = w + pad_w
 *           bottom_diff[n][c][h][w] = dX'[n][c'(c, hp % stride_h, wp % stride_w)][hp / stride_h][wp / stride_w] where the
 *           phase is below (PH, PW) and the index below (H', W'), +0 otherwise: every element of the first n_images
 *           images is written exactly once.
 * With "s2d" = 1 a FLOAT plan in conv_mode SCONV / SCONV_PAR with a stride above 1 in at least one axis and dilation 1,
 * whose bottom, X' and inner weight matrix stay below 2^31 elements and whose Cg' is at most 32767, runs this way:
 * escoin_forward = escoin_s2d_pack_kernel (one pass, zeros included) + the inner plan's forward; the data gradient = the
 * inner plan's backward + escoin_s2d_unpack_kernel.  The inner plan and the X' scratch (also dX') are built by the
 * align; the forward never allocates.  The inner plan gets the options "kernel", "backward_kernel", "tiling_batch",
 * "max_launch_bytes", "dense_threshold_pct", "dense_gate" and "code_loader" and ALONE decides dense or sparse per group,
 * on its own geometry: forcing TILED / JIT fails with ESCOIN_EINVAL where the inner layer does not fit them (KW' > 5,
 * W' > 256, ...).  "backward_kernel" = GENERIC keeps the outer gather kernel, ESCOIN_BWD_MFMA the outer MFMA data
 * gradient; AUTO, TILED, JIT and DENSE go to the inner plan's backward.  The weight, bias and compact gradients and
 * escoin_dense_wgrad read the original bottom and are untouched (the same bits as without the option).  In-place
 * updates (escoin_update_values, escoin_plan_set_values, escoin_solver_step) reach the inner plan's copies and stay in
 * place wherever the inner plan is in-place capable; prune, rewire, set_csr and weight_align rebuild the inner plan.
 * escoin_plan_export_aligned writes the outer CSR and no code section; escoin_plan_import_aligned aligns from it.
 * Everywhere else -- stride 1 in both axes, a dilation (option "s2b" serves the stride-1 ones), a size limit, a double plan, LOWERED_GEMM / LOWERED_SPARSE (a flip
 * of the conv mode rebuilds) -- the plan behaves exactly as with "s2d" = 0, with one exception: in LOWERED_GEMM /
 * LOWERED_SPARSE a layer the option serves in the direct modes, whose own geometry has no tiled kernel, reads a forced
 * "kernel" = TILED / JIT -- the inner plan's kernel -- as AUTO instead of refusing the align, so that a conv_mode flip
 * never leaves the plan unaligned ("backward_kernel" is read as it stands, as with "s2d" = 0).
 * Stats: "s2d" (1 when active), "s2d_scratch_bytes"; "kernel_choice", "bwd_data_kernel", escoin_plan_tiling_info and the
 * other facts about the forward's kernel report the inner plan's; escoin_plan_kernel_name returns
 * "escoin_s2d_pack_kernel + <inner name>".  "device_bytes" and escoin_plan_workspace_bytes count the scratch and the
 * inner plan.  Ordering across streams is the caller's, as for any plan: forward and backward share the scratch.
 * Non-finite input: a non-finite bottom element reaches a zero weight (0 x inf = NaN) only where the inner plan chose
 * its DENSE kernel -- the property the DENSE kernel has without the option; the sparse inner kernels never multiply by a
 * pruned weight, and the padding the pack kernel writes is +0, never a bottom element.
 * escoin_plan_s2d_pack runs the rearrangement alone into the plan's scratch (what escoin_forward runs first), for
 * measuring it; ESCOIN_ESTATE unless stat "s2d" is 1. */
ESCOIN_API int escoin_plan_s2d_pack(escoin_plan *plan, const float *bottom_dev, int n_images, void *stream);

/* ---- Space-to-batch: dilated layers on the stride-1, dilation-1 kernels (option "s2b") -------------------------------
 * A dilated stride-1 convolution is dil_h x dil_w independent undilated convolutions: output pixel (oh, ow) reads only
 * padded input pixels of its own residue class modulo (dil_h, dil_w).  For a descriptor with stride_h = stride_w = 1 let
 * eh = dil_h if KH > 1 else 1, ew = dil_w if KW > 1 else 1 (a dilation on an axis with one tap is no dilation), P = eh * ew,
 * Hp = H + 2 pad_h, Wp = W + 2 pad_w, H' = ceil(Hp / eh), W' = ceil(Wp / ew), OH' = H' - KH + 1 = ceil(OH / eh),
 * OW' = W' - KW + 1 = ceil(OW / ew).  The INNER plan has
 *   N' = N * P images, n' = (n * eh + qh) * ew + qw (the first n_images outer images are the first n_images * P inner
 *   ones), the outer plan's C, M, group, KH x KW and has_bias, an H' x W' image, pad 0, stride 1, dilation 1, fuse_relu = 0;
 *   weights the outer CSR verbatim: same rows, same columns, same value order;
 *   input   X'[n'][c][i][j] = X[n][c][i * eh + qh - pad_h][j * ew + qw - pad_w] inside the image, +0 outside -- the rows
 *           and columns of short residue classes past Hp / Wp included;
 *   T' = inner_forward(X'), the bias in the inner epilogue;
 *   top[n][m][oh][ow] = T'[n'(n, oh % eh, ow % ew)][m][oh / eh][ow / ew], then v > 0 ? v : 0 on a fuse_relu plan (the
 *           epilogues' expression: a NaN becomes 0 as it does there);
 *   G'[n'][m][i][j] = top_diff[n][m][i * eh + qh][j * ew + qw] inside OH x OW, +0 outside; on a fuse_relu plan
 *           top > 0 ? top_diff : 0 there (the expression of the transposed data-gradient path);
 *   dX' = inner_data_gradient(G') (the inner plan has no ReLU and needs no top), and with hp = h + pad_h, wp = w + pad_w
 *           bottom_diff[n][c][h][w] = dX'[n'(n, hp % eh, wp % ew)][c][hp / eh][wp / ew]: every element of the first
 *           n_images images is written exactly once.
 * All P residue classes are always inner images, also where OH < eh leaves some without a top pixel: their G' is all
 * zeros, so bottom pixels no window reads get a zero gradient.
 * With "s2b" = 1 a FLOAT plan in conv_mode SCONV / SCONV_PAR with stride 1 in both axes and P > 1, whose bottom, top, X'
 * and T' each stay below 2^31 elements and whose N * P is at most 65535 (the image index is a grid dimension of the
 * generic kernel and of the backward's kernels), runs this way: escoin_forward = escoin_s2b_pack_kernel (one pass, zeros
 * included) + the inner plan's forward + escoin_s2b_unpack_kernel; the data gradient = escoin_s2b_pack_kernel of top_diff +
 * the inner plan's backward + escoin_s2b_unpack_kernel.  The inner plan and the two scratches (X' / dX' and T' / G') are
 * built by the align; forward and backward never allocate.  The inner plan gets the options "kernel", "backward_kernel",
 * "max_launch_bytes", "dense_threshold_pct", "dense_gate" and "code_loader", and "tiling_batch" times P, and ALONE
 * decides dense or sparse per group, on its own geometry: forcing TILED / JIT fails with ESCOIN_EINVAL where the inner
 * layer does not fit them (KW > 5, W' > 256, ...).  "backward_kernel" = GENERIC keeps the outer gather kernel,
 * ESCOIN_BWD_MFMA the outer MFMA data gradient; AUTO, TILED, JIT and DENSE go to the inner plan's backward.  The weight,
 * bias and compact gradients and escoin_dense_wgrad read the original bottom and are untouched (the same bits as without
 * the option).  In-place updates (escoin_update_values, escoin_plan_set_values, escoin_solver_step) reach the inner plan's
 * copies and stay in place wherever the inner plan is in-place capable; prune, rewire, set_csr and weight_align rebuild
 * the inner plan.  escoin_plan_export_aligned writes the outer CSR and no code section; escoin_plan_import_aligned aligns
 * from it.  Everywhere else -- a stride above 1, P == 1 (dilation 1, a 1x1 kernel), a size limit, a double plan,
 * LOWERED_GEMM / LOWERED_SPARSE (a flip of the conv mode rebuilds) -- the plan behaves exactly as with "s2b" = 0, with the
 * exception "Space-to-depth" states: in the lowered modes a forced "kernel" = TILED / JIT on a layer the option serves
 * in the direct modes is read as AUTO (the dilated geometry has no tiled kernel; the flip must not leave the plan unaligned).
 * Stats: "s2b" (1 when active), "s2b_scratch_bytes" (both scratches); "kernel_choice", "bwd_data_kernel",
 * escoin_plan_tiling_info and the other facts about the forward's kernel report the inner plan's; escoin_plan_kernel_name
 * returns "escoin_s2b_pack_kernel + <inner name> + escoin_s2b_unpack_kernel".  "device_bytes" and
 * escoin_plan_workspace_bytes count the scratches and the inner plan.  Ordering across streams is the caller's, as for
 * any plan: forward and backward share the scratches.
 * Non-finite input: a non-finite bottom element reaches a zero weight (0 x inf = NaN) only where the inner plan chose
 * its DENSE kernel -- the property the DENSE kernel has without the option; the sparse inner kernels never multiply by a
 * pruned weight, and the padding the pack kernel writes is +0, never a bottom element.
 * escoin_plan_s2b_pack runs the forward's first rearrangement alone (the bottom into the X' scratch), escoin_plan_s2b_unpack
 * its last (the T' scratch, whatever it holds, into the top blob), for measuring them; ESCOIN_ESTATE unless stat "s2b" is 1. */
ESCOIN_API int escoin_plan_s2b_pack(escoin_plan *plan, const float *bottom_dev, int n_images, void *stream);
ESCOIN_API int escoin_plan_s2b_unpack(escoin_plan *plan, float *top_dev, int n_images, void *stream);

/* ---- Batch-to-space: inner-product layers on the pointwise kernels (option "b2s") ------------------------------------
 * An InnerProduct layer of K inputs and M outputs is the descriptor {N, C = K, H = W = 1, M, 1x1, stride 1, pad 0}: N
 * images of one pixel.  Every entry point accepts it, but a row of the fast kernels then holds one pixel.  With the batch
 * as the pixel axis the same layer is an ordinary pointwise (1x1) layer.  Let B be the block, a multiple of 4 with
 * 4 <= B <= 256.  The INNER plan has
 *   N' = ceil(N / B) images of 1 x B pixels (the first n_images outer images are the first ceil(n_images / B) inner ones),
 *   the outer plan's C, M, group and has_bias, a 1x1 kernel, pad 0, stride 1, dilation 1 (with one pixel and one tap the
 *   outer stride and dilation are immaterial), fuse_relu = 0;
 *   weights the outer CSR verbatim: same rows, same columns, same value order;
 *   input   X'[n'][c][j] = bottom[n' * B + j][c] for n' * B + j < n_images, +0 otherwise;
 *   T' = inner_forward(X') over ceil(n_images / B) inner images, the bias in the inner epilogue;
 *   top[n][m] = T'[n / B][m][n % B], then v > 0 ? v : 0 on a fuse_relu plan (the epilogues' expression);
 *   G'[n'][m][j] = top_diff[n][m] with n = n' * B + j; on a fuse_relu plan top[n][m] > 0 ? top_diff[n][m] : 0; +0 past
 *           n_images;
 *   the WHOLE backward is the inner plan's, on (X', G') -- where "b2s" departs from "s2d" / "s2b":
 *           bottom_diff[n][c] = dX'[n / B][c][n % B] with dX' = inner_data_gradient(G'); the weight, bias and compact
 *           gradients and escoin_dense_wgrad are the inner plan's own.  weight_diff (M x Cg), values_diff (the same entry
 *           order) and bias_diff have the same layout on both plans: the caller's pointers go straight through, += included.
 *           The padding positions are +0 in both operands and add exact zeros.  The outer plan builds no backward state.
 * Images at or past n_images are neither read nor written on the caller's side, and a padding position is +0 written by the
 * pack kernel, never a bottom element: image n reaches only image n's outputs, also on the inner DENSE kernel.
 * With "b2s" = 1 a FLOAT plan in conv_mode SCONV / SCONV_PAR with H = W = 1, KH = KW = 1 and pad 0, of any group, whose
 * bottom, top, X' and T' each stay below 2^31 elements and whose N' is at most 65535, runs this way: escoin_forward =
 * escoin_b2s_pack_kernel (an LDS-staged transpose, one pass, zeros included) + the inner plan's forward +
 * escoin_b2s_unpack_kernel; escoin_backward / escoin_backward_values = escoin_b2s_pack_kernel of the bottom (where a weight
 * gradient is asked for) and of top_diff + the inner plan's backward + escoin_b2s_unpack_kernel of dX'.  Where both "b2s"
 * and "s2d" are set on a one-pixel layer whose descriptor names a stride, "b2s" serves it.
 * The block: B = 64 (the block that won or tied the sweep of profiles/b2s_mi355x.md on every layer, at batch 256 and at
 * batch 32, where it is half padding); where that gives more than 65535 inner images, the smaller of 128 and 256 that does
 * not.  "b2s_block" forces it.
 * The inner plan and three scratches (X', T' / G', and dX', which must not alias X' within one inner call) are built by the
 * align; the inner plan's backward state by the first backward; after these forward and backward never allocate.  The
 * inner plan gets the options "kernel", "backward_kernel", "wgrad_kernel", "wgrad_channel_block", "max_launch_bytes",
 * "dense_threshold_pct", "dense_gate" and "code_loader" as they stand, and "tiling_batch" in inner images (ceil(tiling_batch
 * / B)), and ALONE decides dense or sparse per group, on its own geometry; forcing TILED / JIT, or a backward or weight-gradient
 * kernel, fails with ESCOIN_EINVAL where the inner layer does not fit it.  In-place updates (escoin_update_values,
 * escoin_plan_set_values, escoin_solver_step) reach the inner plan's copies and stay in place wherever the inner plan is
 * in-place capable; prune, rewire, set_csr and weight_align rebuild the inner plan.  escoin_plan_export_aligned writes the
 * outer CSR and no code section; escoin_plan_import_aligned aligns from it.  Everywhere else -- H * W > 1, a kernel above 1x1,
 * a pad, a size limit, a double plan, LOWERED_GEMM / LOWERED_SPARSE (a flip of the conv mode rebuilds) -- the plan behaves
 * exactly as with "b2s" = 0, with the exception "Space-to-depth" states for a forced "kernel" = TILED / JIT in the lowered modes.
 * Results: where the inner plan runs a sparse kernel an element's sum order is a function of the pattern, so the results
 * depend on neither B nor n_images; with the generic kernel inside they equal the plan without the option bit for bit; the
 * inner DENSE kernel may split K differently per shape and is held to the error bound.
 * Stats: "b2s" (1 when active), "b2s_block" (the B in use), "b2s_scratch_bytes" (the three scratches); "kernel_choice",
 * the "bwd_*" / "wgrad_*" / "dgrad_*" facts, escoin_plan_tiling_info and the other facts about the kernels report the inner
 * plan's; escoin_plan_kernel_name returns "escoin_b2s_pack_kernel + <inner name> + escoin_b2s_unpack_kernel".
 * "device_bytes" and escoin_plan_workspace_bytes count the scratches and the inner plan.  Ordering across streams is the
 * caller's, as for any plan: forward and backward share the scratches.
 * escoin_plan_b2s_pack / escoin_plan_b2s_unpack run one transpose alone on the CALLER's buffers, for measuring and testing:
 * top_side = 0 is the bottom side (CH = C), 1 the top side (CH = M).  pack reads n_images x CH floats of src_dev (and of
 * mask_dev, where not NULL: the value is mask > 0 ? src : 0) and writes the ceil(n_images / B) x CH x B first floats of
 * dst_dev; unpack reads those of src_dev and writes n_images x CH floats of dst_dev, through ReLU if relu != 0.
 * ESCOIN_ESTATE unless stat "b2s" is 1; ESCOIN_EINVAL for NULL buffers or n_images outside [0, N]. */
ESCOIN_API int escoin_plan_b2s_pack(escoin_plan *plan, const float *src_dev, const float *mask_dev, float *dst_dev, int top_side,
                         int n_images, void *stream);
ESCOIN_API int escoin_plan_b2s_unpack(escoin_plan *plan, const float *src_dev, float *dst_dev, int top_side, int relu, int n_images,
                         void *stream);

/* ---- Deconvolution: Caffe's DeconvolutionLayer on the stride-1 kernels (option "deconv") ---------------------------------
 *   DeconvolutionLayer<Dtype>   deconv_layer.cpp: forward = the base layer's backward_*_gemm, backward = forward_*_gemm +
 *                               weight_*_gemm; compute_output_shape at dilation 1
 * escoin_plan_set_option(plan, "deconv", 1) before the align (default 0; other values ESCOIN_EINVAL; after an align
 * ESCOIN_ESTATE, as for "s2d").  The descriptor is then read as a Deconvolution layer's: N, C (bottom channels), H x W (the
 * bottom image), M (num_output), KH x KW, pad, stride, group, has_bias, fuse_relu.  The top is OH = stride_h (H - 1) + KH -
 * 2 pad_h, OW likewise (escoin_deconv_out_shape).  blobs_[0] is C x Mg x KH x KW with Mg = M / group -- Caffe's shape: its
 * conv_out_channels_ is the bottom's channel count.  The CSR is per conv group, rows = the group's Cg bottom channels,
 * column = ml KH KW + kr KW + kc ascending; escoin_plan_get_csr, set_csr, nnz, set_values, values_diff and the compact entry
 * order all use it (it is the CSR of the MIRROR convolution, M <-> C and H x W <-> OH x OW, whose backward this layer is).
 * With m = g Mg + ml and c = g Cg + cl:
 *   top[n][m][oh][ow] = bias[m] + sum over (cl, kr, kc) in the pattern of X[n][c][h][w] * Wd[c][ml][kr][kc]
 *                       where oh + pad_h = h stride_h + kr and ow + pad_w = w stride_w + kc, (h, w) inside H x W,
 * then v > 0 ? v : 0 on a fuse_relu plan (the epilogues' expression: a NaN becomes 0).
 * The decomposition.  Let sh = stride_h, sw = stride_w, P = sh sw, KH' = ceil(KH / sh), KW' = ceil(KW / sw), H' = H + KH' - 1,
 * W' = W + KW' - 1.  The INNER plan has the outer N, C, H x W and group; M' = M P channels, m' = (m sh + ph) sw + pw (a conv
 * group's channels stay contiguous); a KH' x KW' kernel, pad (KH' - 1, KW' - 1), stride 1, dilation 1; has_bias as the outer
 * plan, fuse_relu = 0; its top is H' x W'.  Entry (c, ml, kr, kc) is the entry of row m'(m, kr % sh, kc % sw) at column
 * cl KH' KW' + (KH' - 1 - kr / sh) KW' + (KW' - 1 - kc / sw): an injective map, so the nonzero count and the FLOPs of the
 * sparse walk do not change.  All P phases are inner channels, those that own no tap (sh > KH) included, with empty rows.
 *   forward   T' = inner_forward(X, bias = NULL) on the caller's bottom itself (no pack), then escoin_d2s_unpack_kernel:
 *             top[n][m][oh][ow] = T'[n][m'(m, hp % sh, wp % sw)][hp / sh][wp / sw] + bias[m], hp = oh + pad_h, wp = ow + pad_w,
 *             then the ReLU -- one pass, every element of the first n_images images written exactly once, images past
 *             n_images untouched;
 *   backward  (escoin_backward, escoin_backward_values) escoin_d2s_pack_kernel: G'[n][m'][i][j] = top_diff[n][m][i sh + ph -
 *             pad_h][j sw + pw - pad_w] inside OH x OW (top > 0 ? top_diff : 0 there on a fuse_relu plan), +0 outside; then
 *             the inner plan's backward with bottom = X, top_diff = G' and the caller's bottom_diff pointer.  The inner
 *             compact weight gradient is carried to the outer entry order through the map (values_diff) or scattered into
 *             weight_diff in C x Mg x KH x KW layout; bias_diff[m] takes the inner bias gradients of its P phases, added in
 *             ascending phase order by one lane per m.  No atomics: the bits depend on the geometry, the pattern and
 *             n_images only; every gradient keeps the accumulate / overwrite contract of a convolution plan.
 * The inner plan holds the only forward copy of the weights.  escoin_update_values, escoin_plan_set_values and
 * escoin_solver_step reach its copies in place through the map and stay capturable; weight_align, set_csr and
 * import_aligned rebuild; escoin_plan_export_aligned writes the outer CSR and no code section.  The inner plan gets the
 * options "kernel", "backward_kernel", "wgrad_kernel", "wgrad_channel_block", "tiling_batch", "max_launch_bytes",
 * "dense_threshold_pct", "dense_gate", "code_loader" and "conv_mode" and ALONE decides generated code, stream, dense or
 * generic per group; forcing TILED / JIT where the inner layer does not fit them fails with ESCOIN_EINVAL.  T' and G' share
 * one scratch, allocated by the align with the two small gradient scratches: forward and backward never allocate (but for
 * the inner plan's backward state, at the first backward).
 * There is no kernel of the plan's own to fall back to: a layer the rule (align_rules.h d2s_plan) does not serve is refused
 * at the align with ESCOIN_EINVAL and a message naming the reason -- a dilation other than 1; OH or OW < 1; a double plan or
 * any _f64 entry point; top, T' or the inner weight matrix at or above 2^31 elements; M P above 262140 (a grid axis of the
 * inner generic kernel); more than 32767 output channels per group; "deconv" together with "s2d", "s2b" or "b2s".
 * escoin_plan_create itself still reads the descriptor as a convolution's: a layer whose kernel exceeds H + 2 pad (a 1 x 1
 * bottom under a 4 x 4 kernel) is refused there; lifting that is a later change.
 * escoin_plan_prune, escoin_plan_rewire, escoin_dense_wgrad and their _cpu twins return ESCOIN_EINVAL on a "deconv" plan,
 * naming the option: carrying them over is a later change.  The math_functions-level helpers take no plan and know no
 * Deconvolution layer.
 * CPU mode: escoin_weight_align_cpu, escoin_forward_cpu, escoin_backward_cpu, escoin_backward_values_cpu (and
 * escoin_update_values_cpu, escoin_solver_step_cpu) serve a float "deconv" plan by the same decomposition, with host loops
 * for pack and unpack around the library's own CPU kernels.  With the inner plan forced to the generic kernel the device
 * forward is array-equal to the CPU mode's: both keep the reference's summation order, and the bias is one more rounding in
 * the unpack on both sides.
 * Stats: "deconv" (1 when active), "deconv_scratch_bytes" (the T' / G' scratch); "kernel_choice", the "bwd_*" / "wgrad_*" /
 * "dgrad_*" facts and escoin_plan_tiling_info report the inner plan's; escoin_plan_kernel_name is "<inner name> +
 * escoin_d2s_unpack_kernel"; "device_bytes" and escoin_plan_workspace_bytes count the scratches and the inner plan.
 * escoin_plan_d2s_unpack / escoin_plan_d2s_pack run one kernel alone, for measuring and testing: unpack writes the first
 * n_images images of top_dev from t_dev (NULL: the plan's scratch) + bias_dev (may be NULL), through ReLU on a fuse_relu
 * plan; pack writes G' to g_dev (NULL: the plan's scratch) from top_diff_dev, gated by top_dev > 0 on a fuse_relu plan.
 * ESCOIN_ESTATE unless stat "deconv" is 1. */
ESCOIN_API int escoin_deconv_out_shape(const escoin_conv_desc *desc, int *out_h, int *out_w);
ESCOIN_API int escoin_plan_d2s_unpack(escoin_plan *plan, const float *t_dev, const float *bias_dev, float *top_dev, int n_images,
                           void *stream);
ESCOIN_API int escoin_plan_d2s_pack(escoin_plan *plan, const float *top_diff_dev, const float *top_dev, float *g_dev, int n_images,
                         void *stream);

/* Integer facts about an aligned plan (negative = error): "align_us" wall time of the last
 * weight_align / set_csr / import_aligned, "code_bytes" generated machine code on the device,
 * "device_bytes", "import_fast", "code_direct" (1: the plan's generated code sits in executable device memory the library
 * filled itself, 0: in a module the HIP loader loaded -- option "code_loader"), "cpu_channel_block" / "cpu_images_per_job"
 * (what the last escoin_forward_cpu used), "jit_rows", "jit_records", "lds_bytes", "workgroup_columns",
 * "body_variant" (the compiled body the last tiled launch ran: 0 generic, 1 chained -- option "body_variant"),
 * "code_touchers" (the code-touch stride of the last tiled launch -- option "code_touchers") and "touch_lines_per_launch"
 * (the line requests of that launch's code touches, counted on the host from its grid and stride: every wave's first-unit
 * touch and the touches of each unit of each tile, 64 lines in an elected workgroup and 1 elsewhere; 0 without touches),
 * "kernel_choice" (the ESCOIN_KERNEL_* id AUTO resolved to for the sparse groups), "small_launch_rule" (KERNEL_AUTO's
 * rule for pointwise launches under 64 MFLOP that fit one round of workgroups -- the reference's SCONV mode runs
 * image by image, conv_layer.cu:16-26 --: 0 not considered, 1 kept generated code, 2 took the generic kernel (decided
 * from the tiling before any code is generated or loaded); a function of the options, the weights, the batch and the
 * device MODEL -- its CU count and whether generated code is available -- never of a timing: the same in every process
 * on the same kind of device),
 * "deal_slowest_over_mean_x1000" / "deal_worst_block_x1000" (generated-code plans aligned from weights: how evenly
 * WeightAlign dealt the output channels over the waves that meet at a block's barrier -- slowest wave / mean wave,
 * weighted over all blocks, and the worst single block, x 1000; 0 for a plan restored from a persisted code object),
 * "streamk" / "streamk_gave_up"
 * (dense kernel; a give-up also makes the next escoin_forward on the plan fail with ESCOIN_EHIP),
 * "dense_variant" (which instantiation and store path the plan's last dense launch took: output-channel rows per wave
 * (1: 64-row tiles, 2: 128-row tiles) + 4 if the pointwise operand was staged 16 bytes at a time + 8 if the top was
 * stored 16 bytes at a time + 16 if K was split across workgroups; 0 before the first dense launch). */
ESCOIN_API long escoin_plan_stat(const escoin_plan *plan, const char *key);

/* Name of the device kernel the plan launches (the symbol rocprofv3 reports). */
ESCOIN_API const char *escoin_plan_kernel_name(const escoin_plan *plan);

/* One line describing how the plan's fast kernel tiles the layer (channels per wave, workgroup columns,
 * images per tile, quads per lane, input-channel blocks, plane buffers, generated code or weight
 * stream); "" for plans that run the generic / dense / lowered kernel.  Diagnostics only: the
 * reference has no counterpart (its kernels are fixed-shape, math_functions.cu:524-587).  The
 * string lives as long as the plan and changes with weight_align / set_csr / set_option. */
ESCOIN_API const char *escoin_plan_tiling_info(const escoin_plan *plan);

/* Forward_gpu body for one bottom/top pair, whole batch, asynchronous on `stream`:
 *   top[n][oc] = sconv(bottom[n], CSR)[oc] (+ bias[oc]) (then ReLU if fuse_relu)
 * bottom: n_images x C x H x W, top: n_images x M x OH x OW, bias: M floats or NULL.
 * bias may be NULL even when has_bias was set (the reference dereferences blobs_[1]
 * unconditionally, base_conv_layer.cpp:648 -- not copied).  n_images <= desc.N.
 * Non-finite input: the sparse kernels (generic, LDS stream, DMA stream, generated code, csrmm, and the sparse inner
 * kernels of options "s2d" / "s2b") never multiply by a pruned weight and mask by select, never by multiplication: a NaN
 * or an infinity in the bottom reaches exactly the top elements that a CSR entry reads it for, an infinity with the sign
 * of the one entry that reads it; every other element is what it is without it.  The DENSE kernel (KERNEL_DENSE,
 * LOWERED_GEMM, the dense conv groups of a mixed plan) reads every tap of the element's conv group: pruned positions give
 * 0 x inf = NaN there.  An element of an image at or past n_images is never read.  Every epilogue's ReLU is
 * v > 0 ? v : 0 (or max(v, 0), which returns the other operand for a NaN): a NaN and -inf become +0.
 * Subnormal numbers: bottom elements, weights, the bias and results in the subnormal range are kept -- no kernel of the
 * forward, the backward or the solver step flushes them to zero (the compiled kernels and the generated code run with
 * the float denormal mode "preserve"; the matrix-core kernels' A and B operands follow that mode, their accumulators
 * never flush).  A [top > 0] mask therefore lets the gradient of a positive subnormal top through. */
ESCOIN_API int escoin_forward(escoin_plan *plan, const float *bottom_dev, const float *bias_dev,
                   float *top_dev, int n_images, void *stream);

/* ---- math_functions-level entry points (drop-ins for the reference's GPU helpers,
 * include/caffe/util/math_functions.hpp:194-230).  They operate on the reference's own
 * data layout (shared-halo padded input, stretched CSR) so a Caffe-HIP tree can call
 * them from an unmodified base_conv_layer.cpp. ------------------------------------ */

/* caffe_gpu_sconv<float>, math_functions.cu:590-704 (bias applied iff FUSE_RELU, as
 * there: :215,421 vs :282).  `input` is the padded image(s), per-image stride
 * ifmap_size*num_groups floats (math_functions.cu:566).  Like the reference's kernel it reads
 * the last row's right padding out of the floats that FOLLOW the row; the reference's buffer
 * (base_conv_layer.cpp:71) has those behind the last channel only when pad_h >= 1 -- with
 * pad_h == 0 < pad_w the caller must provide pad_w zero floats more behind the last image
 * (the layer-level path, escoin_forward, needs no padded buffer and has no such case). */
ESCOIN_API int escoin_gpu_sconv(int fuse_relu, int num, const float *input, int ifmap_size,
                     const int *rowptr, const int *colidx, const float *values,
                     const float *bias, int height, int width, int pad_h, int pad_w,
                     int stride_h, int stride_w, int dilation_h, int dilation_w,
                     int kernel_h, int kernel_w, float *output, int num_oc, int num_groups,
                     void *stream);

/* caffe_gpu_stretch, math_functions.cu:706-727 (in place on device colidx). */
ESCOIN_API int escoin_gpu_stretch(const int *rowptr, int *colidx, int M, int height, int width,
                       int pad_h, int pad_w, int kernel_h, int kernel_w, void *stream);

/* copy_input_data<float>, math_functions.cu:729-766: dense image -> padded layout. */
ESCOIN_API int escoin_copy_input_data(float *dst, const float *src, int num_channels, int height,
                           int width, int pad_h, int pad_w, void *stream);

/* caffe_gpu_sparse_csrmm<float>, math_functions.cu:48-62 (cusparseScsrmm2 + cublasSgeam there):
 * C[M x N] = alpha * A_csr[M x K] * B[K x N] + beta * C, all row-major on the device, 0-based
 * CSR with ascending columns.  No transpose scratch: C comes out row-major directly.  The
 * LOWERED_SPARSE comparator (conv_mode 1: im2col + this) is built on it; it is a baseline to
 * measure the direct path against, not the product path. */
ESCOIN_API int escoin_gpu_sparse_csrmm(int M, int N, int K, int nnz, float alpha, const float *values,
                            const int *rowptr, const int *colidx, const float *B, float beta,
                            float *C, void *stream);

/* caffe_gpu_sparse_dense2csr<float>, math_functions.cu:103-152: device dense M x N ->
 * device CSR (0-based, ascending columns); *nnz_total written on the host. */
ESCOIN_API int escoin_gpu_sparse_dense2csr(int M, int N, const float *A, int *nnz_per_row,
                                float *A_nonzero_buf, int *A_idx_pointer_buf,
                                int *A_nonzero_idx_buf, int *nnz_total, void *stream);

/* ---- Dtype = double on the device (conv_layer.cu:75; math_functions.cu:696-704,765-766) ----------------------
 * Same contracts as the float entry points above.  escoin_forward_f64 runs the order-preserving generic kernel
 * (one lane per output pixel, CSR order, fp64 fused multiply-add) in every conv_mode: its results are bit-identical to
 * caffe_cpu_sconv<double>'s.  The aligned-form export / import is defined for float plans only. */
ESCOIN_API int escoin_weight_align_f64(escoin_plan *plan, const double *dense_w, int w_on_device, void *stream);
ESCOIN_API int escoin_plan_set_csr_f64(escoin_plan *plan, const int *rowptr, const int *colidx, const double *values,
                            const int *nnz_per_group, void *stream);
ESCOIN_API int escoin_plan_get_csr_f64(const escoin_plan *plan, int *rowptr, int *colidx, double *values, int stretched);
ESCOIN_API int escoin_forward_f64(escoin_plan *plan, const double *bottom_dev, const double *bias_dev, double *top_dev,
                       int n_images, void *stream);
/* caffe_gpu_sconv<double>, copy_input_data<double>, caffe_gpu_sparse_csrmm<double>, caffe_gpu_sparse_dense2csr<double> */
ESCOIN_API int escoin_gpu_sconv_f64(int fuse_relu, int num, const double *input, int ifmap_size, const int *rowptr,
                         const int *colidx, const double *values, const double *bias, int height, int width,
                         int pad_h, int pad_w, int stride_h, int stride_w, int dilation_h, int dilation_w,
                         int kernel_h, int kernel_w, double *output, int num_oc, int num_groups, void *stream);
ESCOIN_API int escoin_copy_input_data_f64(double *dst, const double *src, int num_channels, int height, int width,
                               int pad_h, int pad_w, void *stream);
ESCOIN_API int escoin_gpu_sparse_csrmm_f64(int M, int N, int K, int nnz, double alpha, const double *values,
                                const int *rowptr, const int *colidx, const double *B, double beta, double *C,
                                void *stream);
ESCOIN_API int escoin_gpu_sparse_dense2csr_f64(int M, int N, const double *A, int *nnz_per_row, double *A_nonzero_buf,
                                    int *A_idx_pointer_buf, int *A_nonzero_idx_buf, int *nnz_total, void *stream);

/* ---- Caffe::CPU mode (Caffe::set_mode(Caffe::CPU)): host entry points, no HIP device needed ---------------------
 *   ConvolutionLayer<Dtype>::Forward_cpu          conv_layer.cpp:25-63
 *     -> BaseConvolutionLayer::forward_cpu_sconv  base_conv_layer.cpp:569-661 (pad copy :601-620, groups :626-658)
 *        -> caffe_cpu_sconv<Dtype>                math_functions.cpp:128-176
 *     -> forward_cpu_bias                         base_conv_layer.cpp:663-669
 *   WeightAlign, CPU branch                       base_conv_layer.cpp:46-107
 * Implemented in this library (csrc/sconv_cpu.cpp, sconv_cpu_kernel.cpp: AVX2 / AVX-512 register tiles over the
 * shared-halo layout, a team of host threads over images and output channels).  Every output is
 * fma(value_j, input_j, sum) over its row's nonzeros in CSR order from zero, + bias once afterwards, then ReLU --
 * the arithmetic of the reference's loop nest, so results are BIT-IDENTICAL to caffe_cpu_sconv + forward_cpu_bias for
 * float and for double, whatever the thread count.  Differences kept on purpose: the density gate that sends a layer
 * to the dense GEMM above 50 % density (base_conv_layer.cpp:572-577) is not reproduced (the sparse kernel computes the
 * same sums), every Caffe::ConvMode takes this path (the reference's Forward_cpu uses it for SCONV only), and bias
 * may be NULL. */

/* Which flavour of the host kernel this machine runs ("escoin_cpu_sconv_avx512" / "..._avx2"). */
ESCOIN_API const char *escoin_cpu_kernel_name(void);
/* Pins the flavour for the calls that follow, process-wide: "avx2", "avx512" (ESCOIN_ENODEVICE when this CPU lacks it)
 * or "auto" (what the CPU reports; the default).  Results are bit-identical in every flavour; the tests use this to run
 * both on one machine. */
ESCOIN_API int escoin_cpu_kernel_select(const char *which);

/* WeightAlign() in CPU mode: dense blobs_[0] on the host -> the plan's host CSR.  No device work; a plan aligned this
 * way serves escoin_forward_cpu only (escoin_forward needs escoin_weight_align).  Conversely escoin_forward_cpu also
 * works on a plan aligned by escoin_weight_align / set_csr / import_aligned: the CSR is on the host either way. */
ESCOIN_API int escoin_weight_align_cpu(escoin_plan *plan, const float *dense_w);
ESCOIN_API int escoin_weight_align_cpu_f64(escoin_plan *plan, const double *dense_w);

/* Forward_cpu body for one bottom/top pair, whole batch, host pointers; returns when the batch is done.
 * n_threads: host threads to use (<= 0: all the process may run on).  n_images is not bounded by desc.N.
 * The threads are a process-wide pool of parked std::threads, grown on demand; a new one inherits the CPU affinity of
 * the thread whose call started it (a caller pinned to one core -- e.g. by an OpenMP runtime's OMP_PROC_BIND -- gets
 * a pool pinned to that core: widen the mask around the first call if that is not wanted).  Inside that mask a worker
 * moves itself to a core of its own when it starts and takes the whole mask back at once: the team is spread over the
 * cores from the first call, and nothing stays bound (the scheduler may still move it). */
ESCOIN_API int escoin_forward_cpu(escoin_plan *plan, const float *bottom, const float *bias, float *top, int n_images,
                       int n_threads);
ESCOIN_API int escoin_forward_cpu_f64(escoin_plan *plan, const double *bottom, const double *bias, double *top,
                           int n_images, int n_threads);

/* caffe_cpu_sconv<Dtype>, math_functions.cpp:128-176 (declared include/caffe/util/math_functions.hpp:40-47): one conv
 * group of one image on the reference's padded layout with the stretched CSR; `bias` is accepted and ignored, as there.
 * Reads nothing past the last element an output needs; fails with ESCOIN_EINVAL if that lies at or beyond
 * input_padded_len (the reference asserts it, :168; input_padded_len <= 0 skips the check). */
ESCOIN_API int escoin_cpu_sconv(const float *input_padded, int in_channels, int height, int width, int pad_h, int pad_w,
                     int stride_h, int stride_w, int dilation_h, int dilation_w, const int *rowptr,
                     const int *colidx, const float *values, int kernel_h, int kernel_w, const float *bias,
                     float *output, int out_channels, int input_padded_len);
ESCOIN_API int escoin_cpu_sconv_f64(const double *input_padded, int in_channels, int height, int width, int pad_h,
                         int pad_w, int stride_h, int stride_w, int dilation_h, int dilation_w, const int *rowptr,
                         const int *colidx, const double *values, int kernel_h, int kernel_w, const double *bias,
                         double *output, int out_channels, int input_padded_len);

/* caffe_cpu_sparse_dense2csr<Dtype>, the hand loop of math_functions.cpp:92-105 (0-based, ascending columns;
 * argument order as there: values, column indices, row pointers). */
ESCOIN_API int escoin_cpu_sparse_dense2csr(int M, int N, const float *A, float *A_nonzero_buf, int *A_nonzero_idx_buf,
                                int *A_idx_pointer_buf);
ESCOIN_API int escoin_cpu_sparse_dense2csr_f64(int M, int N, const double *A, double *A_nonzero_buf,
                                    int *A_nonzero_idx_buf, int *A_idx_pointer_buf);

/* ---- Backward: ConvolutionLayer::Backward_gpu / Backward_cpu that keeps the sparsity pattern ------------------------
 *   ConvolutionLayer<Dtype>::Backward_gpu            conv_layer.cu:42-73
 *     -> backward_gpu_gemm / weight_gpu_gemm / backward_gpu_bias   base_conv_layer.cpp:859-897
 * The reference's backward is dense (im2col + GEMM): in SCONV mode it writes a dense weight gradient, so a solver step
 * brings pruned weights back while the sparse forward -- which reads the CSR WeightAlign built -- never sees them.  This
 * backward propagates through the plan's CSR nonzeros only and gives a gradient only to the weights the CSR holds: it
 * is consistent with the forward, costs about density x the dense FLOPs, and equals the reference's gradient on
 * unpruned weights.  With the masked gradient plain SGD (momentum, weight decay) and Adam keep a pruned weight at exactly
 * 0, so re-aligning after the update reproduces the pattern.
 *
 * Let G = top_diff, or top_diff x [top > 0] for fuse_relu plans.  For one bottom/top pair, whole batch:
 *   bottom_diff[n][c][h][w]  = sum of value x G[n][oc][oh][ow] over the CSR entries (oc, c, kr, kc) and the output
 *                              pixels with oh*stride_h - pad_h + kr*dil_h = h, ow*stride_w - pad_w + kc*dil_w = w;
 *                              OVERWRITTEN (backward_gpu_gemm: beta 0, then col2im);
 *   weight_diff[oc*Cg*KH*KW + colidx] += sum over (n, oh, ow) of G x bottom[...] (0 outside the image), at the plan's CSR
 *                              positions ONLY -- explicit zeros handed to set_csr included; no other element is read or
 *                              written (a NaN there stays NaN);
 *   bias_diff[oc]            += sum over (n, oh, ow) of G.
 * A NULL output is not computed (propagate_down / param_propagate_down).  bottom is required iff weight_diff != NULL,
 * top iff desc.fuse_relu, top_diff always.  The plan's conv_mode is ignored: all four modes compute the same function.
 * Errors: ESCOIN_ESTATE before an align, on the other Dtype's entry point or (GPU) on another device; ESCOIN_EINVAL for a
 * NULL top_diff, fuse_relu without top, weight_diff without bottom, n_images outside [0, desc.N] (GPU) / < 0 (CPU).
 * Deterministic: for a fixed plan, inputs and n_images the output bits are the same on every call, on any stream and
 * for any n_threads (no float atomics; every sum's order is a function of the geometry and n_images only).
 * The first GPU backward on an aligned plan builds the backward state: the data-gradient path, the weight-gradient
 * reduction slab (chunks of 1024 (n, oh, ow) pixels x nonzeros) and, for fuse_relu plans on the transposed path, a
 * G buffer of desc.N x M x OH x OW.  Later calls allocate and synchronise nothing (they can be captured into a graph);
 * weight_align / set_csr / import_aligned drop the state, escoin_plan_workspace_bytes counts it.
 * Data gradient: on a float plan with stride 1 and pad <= dil x (K - 1) a forward sparse convolution of G with the
 * transposed, flipped weights, run by an internal plan (C' = M, H' x W' = OH x OW, M' = C, pad' = dil x (K - 1) - pad,
 * no bias, no ReLU; it inherits tiling_batch, max_launch_bytes, dense_threshold_pct, dense_gate, code_loader) -- the
 * forward's kernel families; otherwise the order-preserving gather kernel escoin_sconv_bwd_data_kernel, bit-identical
 * to escoin_backward_cpu.  Weight / bias gradient: escoin_sconv_wgrad_partial_kernel (one partial per (chunk, entry))
 * then escoin_sconv_wgrad_sum_kernel (each entry's partials in chunk order, then +=).
 * Option "backward_kernel" (before the align, like the others): AUTO (default) = the transposed plan picks its kernel
 * where it exists; GENERIC = the gather kernel; TILED / JIT / DENSE = that kernel on the transposed plan (the first
 * backward fails with ESCOIN_EINVAL where there is none).
 * ESCOIN_BWD_MFMA (5; a value of "backward_kernel" only -- option "kernel" rejects it; never chosen by AUTO) =
 * escoin_sconv_dgrad_mfma_kernel, for the layers kept dense that have no transposed plan (stride > 1, or pad > dil x
 * (K - 1)).  The bottom pixels split into stride_h x stride_w phases ((h + pad_h) % stride_h, (w + pad_w) % stride_w);
 * inside a phase every pixel has the same contributing taps, so a phase is one stride-1 implicit GEMM
 * dX_phase[Cg x P] = Wt_phase[Cg x Mg*taps] x gather(G)[Mg*taps x P] over the phase's (n, h, w) pixels, run on the fp32
 * matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums) by one workgroup per (phase, 64 phase pixels, 64
 * input channels of a conv group), 32 columns per LDS step, the whole reduction in that workgroup (no split-K, no atomics).
 * A phase without taps (three of the four of a 1x1 stride-2 layer) writes zeros; every bottom element is overwritten
 * once, and images at or past n_images are not touched.  The weights are kept as one transposed dense copy with the
 * columns permuted by phase (zero outside the pattern), which escoin_update_values, escoin_plan_set_values and
 * escoin_solver_step reach in place: after any of them the data gradient equals, bit for bit, that of a fresh plan
 * aligned by set_csr on the new values.  It serves float plans of any stride, pad, dilation, group count and kernel shape
 * with N*H*W, Mg*OH*OW and the matrices' floats (about C*Mg*KH*KW rounded up to 64 channels and 32 columns per phase)
 * below 2^31, H, W, pads and dilated kernel extents below 2^28, at most 65535 phases and 65535 (group, 64-channel tile)
 * pairs; on a double plan or outside these the first backward fails with ESCOIN_EINVAL.  Sum order: per element the live
 * steps of 32 columns ascending (a step is live when its 64 channels x 32 columns hold a CSR entry), inside a step the
 * matrix instruction's own order -- a function of the geometry and the pattern only, not of n_images nor of an image's
 * place in the batch; equality of its bits with the gather kernel's is no part of the contract.  The work is the dense problem restricted to live
 * steps: a pruned position inside a live step contributes 0 x G, so a NON-FINITE G element gives NaN in input channels
 * whose weight for it is pruned, where the gather kernel gives a finite value (the forward's DENSE kernel has the same
 * property towards a non-finite bottom).  The weight / bias gradient paths are untouched and combine with it freely.
 * Stats: "bwd_data_kernel" (ESCOIN_KERNEL_GENERIC = the gather kernel, ESCOIN_BWD_MFMA = the MFMA data-gradient kernel,
 * otherwise the transposed plan's resolved kernel;
 * ESCOIN_ESTATE before the first backward), "bwd_device_bytes" (the phase matrices and their tables included),
 * "dgrad_lds_bytes" (LDS of an MFMA data-gradient workgroup; 0 on the other paths), "bwd_chunks" (chunks the last
 * weight / bias gradient reduced over), "bwd_align_us" (build time of the backward state).
 * Option "wgrad_kernel" (before the align): which stage 1 produces the per-chunk partials of the weight / bias gradient.
 * ESCOIN_WGRAD_ENTRY = escoin_sconv_wgrad_partial_kernel, which reads the bottom from global memory once per nonzero,
 * then escoin_sconv_wgrad_sum_kernel.  ESCOIN_WGRAD_STAGED = escoin_sconv_wgrad_staged_kernel: one workgroup per (chunk,
 * slice of output channels, block of input channels) stages the chunk's padded bottom rows of the block in LDS once;
 * each wave holds G of one output channel for the whole chunk in registers and walks that channel's entries of the block
 * with one LDS read per FMA, reducing across lanes eight entries at a time; then escoin_sconv_wgrad_tree_sum_kernel,
 * which deals the chunk axis over 16 lanes per entry.  It serves float plans with stride 1 (any pad, dilation, group
 * count, KH != KW) whose tile of one input channel fits 64 KiB of LDS; forcing it elsewhere makes the first backward fail
 * with ESCOIN_EINVAL.  ESCOIN_WGRAD_AUTO (default) = the staged kernel where it serves the plan and a cost model of the
 * two kernels -- a function of the geometry, nnz and the device's CU count, never a timing -- has it faster (the model,
 * its fit and its measurements: profiles/backward_mi355x.md).  The two kernels sum in different orders: the low bits of the gradient differ between
 * them, each is deterministic.  The chunks and the slab are the same ("bwd_chunks" keeps its meaning).
 * ESCOIN_WGRAD_MFMA = escoin_sconv_wgrad_mfma_kernel, for layers kept dense (conv1, dense 1x1 layers, groups the forward
 * sends to its MFMA kernel): one workgroup per (chunk, 64 output channels of a conv group, 64 columns of its Cg*KH*KW
 * weight matrix) multiplies G[64 x pixels] by the im2col view of the bottom [pixels x 64] on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums), 32 pixels per LDS step, and writes the tile's elements that
 * are CSR entries to the slab; tiles without entries do no work; then escoin_sconv_wgrad_tree_sum_kernel.  Never chosen by
 * AUTO.  It serves float plans of any stride, pad, dilation, group count and kernel shape with N*OH*OW, M*Cg*KH*KW and
 * Cg*H*W below 2^31 (H, W, pads and dilated kernel extents below 2^28), at most 65535 (group, 64-channel tile) pairs and
 * 65535 column tiles; forcing it on a double plan or
 * outside these makes the first backward fail with ESCOIN_EINVAL.  Sum order: per (chunk, entry) the chunk's live
 * pixels ascending, 32 per step and two per matrix instruction, then the chunks by the tree sum -- a function of the
 * geometry and n_images only; its low bits differ from the other two kernels'.  Only CSR positions are written (a NaN
 * elsewhere stays NaN, explicit zeros receive their gradient).  Its bias gradient is the entry kernel's, bit for bit:
 * escoin_sconv_wgrad_partial_kernel launched for the bias alone, then escoin_sconv_wgrad_sum_kernel.
 * Option "wgrad_pointwise" (0 or 1, default 0; settable whenever "wgrad_kernel" is, and read when the next backward state
 * is built): with "wgrad_kernel" at ESCOIN_WGRAD_AUTO, a plan the pointwise rule serves runs stage 1 -- weights and bias --
 * by escoin_sconv_wgrad_pointwise_kernel, then escoin_sconv_wgrad_tree_sum_kernel.  A plan the rule does not serve
 * behaves exactly as without the option (same kernel, same bits); a forced "wgrad_kernel" wins over it; AUTO never picks
 * the kernel by itself.  It is not a value of "wgrad_kernel" (4 is refused there).  Served: float plans with KH = KW = 1
 * and pad 0, any stride and group count, with N*OH*OW, C*H*W and nnz below 2^31 and at most 65535 chunks of 1024 pixels
 * (N*OH*OW <= 67 107 840); a double plan is not served.  One workgroup per (tile, chunk), a tile being a slice of a conv
 * group's output channels crossed with a block of its input channels: the tile's G rows and bottom rows go through LDS 32
 * pixels at a time (the ReLU mask and the stride gather applied on the way in), and each lane owns up to 16 of the
 * tile's entries, one accumulator register each.  Sum order: per (chunk, entry) ONE fma chain from +0 over the chunk's
 * pixels in ascending order, in one lane with no cross-lane step (likewise the bias: one lane's chain of additions per
 * chunk and output channel), then the chunks by the tree sum -- a function of the geometry, the pattern's positions and
 * n_images only, whatever the tiling; the low bits differ from the other kernels'.  Only CSR positions are written,
 * explicit zeros receive their gradient, images at or past n_images are not read, a non-finite bottom element reaches the
 * entries of its channel only, and a bias-only call stages no bottom.  Options "b2s" and "deconv" hand the option to
 * their inner plan, which is pointwise for every inner-product layer and for deconvolutions whose kernel does not exceed
 * the stride; "s2d" / "s2b" compute the weight gradient on the outer plan, which the option serves where that plan itself
 * is pointwise (a 1x1 stride-2 layer under "s2d").  Measurements: profiles/wgrad_pointwise_mi355x.md.
 * Option "wgrad_channel_block" (test option, before the align): 0 = as many input channels per staged block as the
 * LDS budget holds, n = at most n; it caps the pointwise kernel's channel block too.  Results do not depend on it.
 * Option "wgrad_pointwise_tile_entries" (test option, before the align; >= 0): 0 = a pointwise tile holds up to 4096
 * entries, n = at most min(n, 4096).  Results do not depend on it.
 * Stats: "wgrad_kernel" (ESCOIN_WGRAD_ENTRY / _STAGED / _MFMA / _POINTWISE: what the last weight / bias gradient ran;
 * ESCOIN_ESTATE before the first one), "wgrad_lds_bytes" (LDS of a staged, an MFMA or a pointwise workgroup; 0 on the
 * entry kernel). */
#define ESCOIN_WGRAD_AUTO 0
#define ESCOIN_WGRAD_ENTRY 1   /* escoin_sconv_wgrad_partial_kernel: one workgroup per (chunk, output channel) */
#define ESCOIN_WGRAD_STAGED 2  /* escoin_sconv_wgrad_staged_kernel: the chunk's bottom staged in LDS */
#define ESCOIN_WGRAD_MFMA 3    /* escoin_sconv_wgrad_mfma_kernel: G x im2col(bottom) on the fp32 matrix cores */
#define ESCOIN_WGRAD_POINTWISE 4 /* escoin_sconv_wgrad_pointwise_kernel (option "wgrad_pointwise"): a value of the stat only */
#define ESCOIN_BWD_MFMA 5      /* option "backward_kernel" only: escoin_sconv_dgrad_mfma_kernel, one gather-GEMM per stride phase */
ESCOIN_API int escoin_backward(escoin_plan *plan, const float *bottom_dev, const float *top_dev, const float *top_diff_dev,
                    float *bottom_diff_dev, float *weight_diff_dev, float *bias_diff_dev, int n_images, void *stream);
ESCOIN_API int escoin_backward_f64(escoin_plan *plan, const double *bottom_dev, const double *top_dev,
                        const double *top_diff_dev, double *bottom_diff_dev, double *weight_diff_dev,
                        double *bias_diff_dev, int n_images, void *stream);
/* Backward_cpu (conv_layer.cpp:65-99): the same function on host pointers, on a plan with a host CSR (any align);
 * n_threads as in escoin_forward_cpu.  Plain loops; the data gradient is bit-identical to the device gather kernel's. */
ESCOIN_API int escoin_backward_cpu(escoin_plan *plan, const float *bottom, const float *top, const float *top_diff,
                        float *bottom_diff, float *weight_diff, float *bias_diff, int n_images, int n_threads);
ESCOIN_API int escoin_backward_cpu_f64(escoin_plan *plan, const double *bottom, const double *top, const double *top_diff,
                            double *bottom_diff, double *weight_diff, double *bias_diff, int n_images, int n_threads);

/* The same backward with the weight gradient in COMPACT form: values_diff holds nnz elements in the order of
 * escoin_plan_get_csr, groups concatenated -- the order escoin_plan_set_values reads, so a solver can run on compact
 * tensors (v -= lr * values_diff; escoin_plan_set_values(v) -- or escoin_solver_step on values_diff, below) and a
 * data-parallel all-reduce moves nnz values, not a
 * blob that is 90-95 % zeros.  values_diff is accumulated (+=); explicit zeros of the CSR receive a gradient; nothing
 * outside the nnz elements is touched.  Everything else is escoin_backward's contract with values_diff in the place
 * of weight_diff (bottom required iff values_diff != NULL, the same errors, determinism, no allocation after the first
 * call).  No new work: stage 2 of the reduction writes entry e to values_diff[e] instead of weight_diff[position of e],
 * so for the same "wgrad_kernel" values_diff equals weight_diff gathered at the CSR positions bit for bit. */
ESCOIN_API int escoin_backward_values(escoin_plan *plan, const float *bottom_dev, const float *top_dev,
                           const float *top_diff_dev, float *bottom_diff_dev, float *values_diff_dev,
                           float *bias_diff_dev, int n_images, void *stream);
ESCOIN_API int escoin_backward_values_f64(escoin_plan *plan, const double *bottom_dev, const double *top_dev,
                               const double *top_diff_dev, double *bottom_diff_dev, double *values_diff_dev,
                               double *bias_diff_dev, int n_images, void *stream);
ESCOIN_API int escoin_backward_values_cpu(escoin_plan *plan, const float *bottom, const float *top, const float *top_diff,
                               float *bottom_diff, float *values_diff, float *bias_diff, int n_images, int n_threads);
ESCOIN_API int escoin_backward_values_cpu_f64(escoin_plan *plan, const double *bottom, const double *top,
                                   const double *top_diff, double *bottom_diff, double *values_diff,
                                   double *bias_diff, int n_images, int n_threads);

/* ---- Weight updates: the second half of a training step -------------------------------------------------------------
 *   Solver::ApplyUpdate -> Net::Update -> Blob::Update (solver.cpp, blob.cpp) changes blobs_[0]; the reference then has
 *   to run WeightAlign again before the sparse forward sees the new weights.
 * A plan computes from COPIES of the weights that WeightAlign made -- the generic kernel's value array, the stream
 * kernel's quads, the dense kernel's padded matrix, 32-bit words inside generated machine code, and the backward state's
 * transposed copies of all of these.  Everything else WeightAlign decides is a function of the sparsity PATTERN and the
 * options, and the masked gradient of escoin_backward keeps the pattern: after a solver step only the values differ.
 * These entry points write the new values into every copy, in place.
 *   dense_w  blobs_[0] (M x C/g x KH x KW).  Only the elements at the plan's CSR positions are read; every other element
 *            is ignored (it is 0 under the masked gradient; a NaN there does no harm).  A caller that GREW the pattern
 *            must call escoin_weight_align (or grow it with escoin_plan_rewire, "Rewiring" below).  A kept weight whose new value is exactly 0 stays in the CSR as an explicit
 *            zero (-0.0 stays -0.0).
 *   values   (escoin_plan_set_values) the compact array, nnz elements in the order of escoin_plan_get_csr -- what rank 0
 *            would broadcast after a step instead of a blob.  escoin_backward_values writes its values_diff in the same
 *            order: element e of one is the gradient of element e of the other.
 * The pattern, tiling, kernel choice, channel deal, the generated code's instructions, every device allocation and the
 * backward state stay.  After the call every consumer of the plan -- escoin_forward in all four conv_modes (a later flip
 * to or from LOWERED_GEMM included), escoin_backward's data gradient on the transposed plan or the gather kernel,
 * escoin_plan_get_csr, escoin_plan_export_aligned, escoin_forward_cpu / escoin_backward_cpu -- behaves BIT FOR BIT like a
 * fresh plan with the same options aligned (escoin_plan_set_csr) on the new values at the old pattern.
 * Device source (w_on_device / on_device != 0): one launch of escoin_update_values_kernel (one lane per destination word,
 * one plain store each), asynchronous on `stream`, no host synchronisation.  The FIRST update on an alignment builds the
 * update state (the scatter list: device memory, a synchronisation); so does the first one after the backward state
 * appeared.  Later calls allocate nothing and can be captured into a graph together with escoin_forward and
 * escoin_backward.  Ordering against launches of the plan on OTHER streams is the caller's, as for any buffer.
 * Host source: the host CSR is updated directly, the compact values go through a staging buffer the update state owns,
 * then the same kernel; the call returns when the copy is done.
 * Host mirrors after a device-source update: the plan cannot see a graph replay, so from the first device-source update
 * until the next align (or host-source update) the DEVICE is authoritative.  Everything that reads weights from the host
 * -- get_csr, export_aligned, the CPU entry points, a backward state that is built later, the rebuild a conv_mode flip
 * to or from LOWERED_GEMM does -- first reads the value array back: a copy of nnz values on the stream the last update
 * used, then a wait on that stream (which must therefore still exist, and must not be capturing; after graph REPLAYS the
 * caller synchronises the replay's stream first -- the plan saw the capture, not the replays), then the host CSR and
 * the host's copy of the generated code are patched, so that an exported blob and its content tags carry the new
 * values.  Mixed CPU / GPU use pays that read-back once per device-source update followed by a host read: alternate
 * escoin_forward_cpu with device-source updates and every step copies nnz values and waits for the stream.
 * Fallback (correct, slow; stat "update_fast" = 0): where the in-place path does not exist the update rebuilds the device
 * side from the host CSR with the new values, exactly as escoin_plan_set_csr would -- it synchronises, allocates and
 * drops the backward state; only update_fast = 1 calls are capturable.  Two plan kinds take it: generated code that the
 * HIP module loader placed (stat "code_direct" = 0: its memory is the loader's), and a plan restored by the fast import
 * (its blob carries code but no value map; the rebuild produces one, so the NEXT update is in place).
 * escoin_update_values_cpu[_f64]: for plans aligned by escoin_weight_align_cpu only (host CSR, no device side); no HIP
 * call.  On a device-aligned plan it returns ESCOIN_ESTATE: escoin_update_values(..., w_on_device = 0, ...) updates both
 * sides.
 * Errors: ESCOIN_EINVAL for a NULL argument; ESCOIN_ENODEVICE for the GPU entry points without a device (no silent CPU
 * fallback, as everywhere); ESCOIN_ESTATE before an align, on the other Dtype's entry point, on another device.
 * Stats: "update_fast" (1: the last update was the in-place scatter, 0: it took the fallback), "update_count" (updates
 * since the plan was created), "update_destinations" (words one update writes), "upd_device_bytes" (the update state's
 * device memory; escoin_plan_workspace_bytes = device_bytes + bwd_device_bytes + upd_device_bytes). */
ESCOIN_API int escoin_update_values(escoin_plan *plan, const float *dense_w, int w_on_device, void *stream);
ESCOIN_API int escoin_update_values_f64(escoin_plan *plan, const double *dense_w, int w_on_device, void *stream);
ESCOIN_API int escoin_plan_set_values(escoin_plan *plan, const float *values, int on_device, void *stream);
ESCOIN_API int escoin_plan_set_values_f64(escoin_plan *plan, const double *values, int on_device, void *stream);
ESCOIN_API int escoin_update_values_cpu(escoin_plan *plan, const float *dense_w);
ESCOIN_API int escoin_update_values_cpu_f64(escoin_plan *plan, const double *dense_w);

/* ---- Solver step: the solver's element-wise rule fused into the in-place update ----------------------------------------
 *   SGDSolver::ApplyUpdate = Normalize, Regularize, ComputeUpdateValue (sgd_solver.cpp:118-204 and one element-wise kernel
 *   per rule: sgd_solver.cu:7-12, nesterov_solver.cu:7-14, adam_solver.cu:7-15), then Net::Update -> Blob::Update.
 * Every operand of that kernel is at hand for a lane that holds one CSR entry of the plan, so a training step of a pruned
 * layer is escoin_forward -> escoin_backward_values -> escoin_solver_step: three calls, nothing of the caller's between
 * them, and the same three nodes in a graph.
 *   diff      the gradient: values_diff (nnz elements, escoin_plan_get_csr's order; diff_is_dense = 0) or a blobs_[0]-
 *             shaped weight_diff (diff_is_dense = 1), read -- and with clear_diff set to +0 -- at the CSR positions only
 *   history   SGD / Nesterov: h; Adam: m.  history2: Adam's v, otherwise NULL (ignored).  Caller-owned arrays of nnz
 *             elements in get_csr's order, like every blob of this ABI: snapshots, all-reduces and re-alignments stay the
 *             caller's business.
 *   dense_w   NULL, or blobs_[0]: the new values are also written there, at the CSR positions only
 * The plan's value array (every plan kind keeps one) is the current weight w.  The pointers must not overlap each other
 * or the plan's memory.
 * Arithmetic, per CSR entry e, every operation in the plan's Dtype, each rounded once, never contracted into a fused
 * multiply-add; the hyper-parameters (and 1 + momentum, 1 - beta1, 1 - beta2) are converted / formed in Dtype once per call:
 *   g = diff[e];                      if diff_scale != 1: g = diff_scale * g
 *   L2: g = g + decay * w             L1: g = g + decay * sign(w)   (sign(+-0) = sign(NaN) = 0; skipped when decay == 0)
 *   SGD:      h' = momentum*h + rate*g;                 u = h'
 *   Nesterov: h' = momentum*h + rate*g;                 u = (1 + momentum)*h' - momentum*h
 *   Adam:     m' = m*beta1 + g*(1 - beta1);  v' = v*beta2 + (g*g)*(1 - beta2);   u = (rate*m') / (sqrt(v') + delta)
 *   w' = w - u
 * The reference's Nesterov and Adam kernels keep `float` temporaries in their double instantiation; that quirk is NOT
 * reproduced: the _f64 entry points compute in double throughout.
 * Effect: escoin_plan_set_values' contract on the new values w' -- every consumer of the plan then behaves bit for bit
 * like a fresh plan aligned by escoin_plan_set_csr on w' at the old pattern, in all four conv_modes and for the backward
 * state's copies; the device is authoritative afterwards and the host mirrors follow as after a device-source update;
 * "update_count" increments, "update_fast" reports the path.  An explicit zero of the pattern is updated like any entry.
 * With nnz == 0 the call returns ESCOIN_OK without a launch; diff, history and history2 (arrays of 0 elements) may then
 * be NULL.
 * One launch of escoin_solver_step_kernel, one lane per CSR ENTRY: the lane reads w, diff, h (h2), computes the rule once,
 * writes h (h2), dense_w, the cleared diff, and stores w' to each of the entry's destinations (the value array, the code
 * word or stream quad, the dense matrix, the backward state's copies) through an entry-major view of the update state's
 * destination list.  No atomics; no lane reads a word another lane of the launch writes.  The view is built with the
 * first solver step on an alignment (and once more when the backward state appears): device memory, a synchronisation;
 * later steps allocate and synchronise nothing and can be captured.  rate_dev lets a captured step follow an lr policy.
 * Plans without an in-place path (see "Fallback" above) run the same kernel with the value array as the only destination
 * and then rebuild from it: update_fast = 0, not capturable; the next step on the rebuilt plan is in place.
 * escoin_solver_array_step: the same rule on a plain array (`data` is w and the only destination): the bias, any blob.
 * The _cpu entry points are plain host loops with the same bits: escoin_solver_step_cpu for plans aligned by
 * escoin_weight_align_cpu only (as escoin_update_values_cpu), all pointers host pointers, rate_dev included.
 * Errors: ESCOIN_EINVAL for a NULL desc, a NULL diff / history on a plan with entries (array step: data, or n < 0), an
 * unknown type or regularization, Adam without history2 on a plan with entries; ESCOIN_ENODEVICE for the device entry points without a device; ESCOIN_ESTATE before an align, on
 * the other Dtype's entry point, on another device, and for escoin_solver_step_cpu on a device-aligned plan. */
#define ESCOIN_SOLVER_SGD 0        /* sgd_solver.cu:7-12      */
#define ESCOIN_SOLVER_NESTEROV 1   /* nesterov_solver.cu:7-14 */
#define ESCOIN_SOLVER_ADAM 2       /* adam_solver.cu:7-15     */
#define ESCOIN_REG_NONE 0
#define ESCOIN_REG_L2 1            /* sgd_solver.cpp:155-160  */
#define ESCOIN_REG_L1 2            /* sgd_solver.cpp:161-168  */
typedef struct escoin_solver_desc {
  int type, regularization;
  double rate;        /* the kernel's local_rate; for Adam the corrected_local_rate (adam_solver.cpp:39-41,80): the caller
                         applies lr_mult and the bias correction, the library knows no iteration count */
  double momentum;    /* SGD / Nesterov momentum; Adam beta1 */
  double momentum2;   /* Adam beta2 */
  double delta;       /* Adam eps_hat */
  double decay;       /* local_decay = weight_decay * decay_mult; 0 = no regularisation term */
  double diff_scale;  /* multiplies the gradient first: Normalize's 1/iter_size, ClipGradients' scale, 1/world_size;
                         exactly 1.0 = no multiplication */
  const void *rate_dev; /* NULL, or a device (host for _cpu) pointer to ONE Dtype that replaces `rate`, read by the kernel:
                           a captured step then follows an lr policy / Adam's correction without re-capture */
  int diff_is_dense;  /* 0: diff is values_diff (nnz, get_csr's order); 1: diff is a blobs_[0]-shaped weight_diff, read
                         (and cleared) at the CSR positions only.  Ignored by the array step. */
  int clear_diff;     /* 1: the elements of diff that were read are set to +0 (Net::ClearParamDiffs for the next +=) */
} escoin_solver_desc;
ESCOIN_API int escoin_solver_step(escoin_plan *plan, const escoin_solver_desc *desc, float *diff, float *history,
                       float *history2, float *dense_w, void *stream);
ESCOIN_API int escoin_solver_step_f64(escoin_plan *plan, const escoin_solver_desc *desc, double *diff, double *history,
                           double *history2, double *dense_w, void *stream);
ESCOIN_API int escoin_solver_step_cpu(escoin_plan *plan, const escoin_solver_desc *desc, float *diff, float *history,
                           float *history2, float *dense_w);
ESCOIN_API int escoin_solver_step_cpu_f64(escoin_plan *plan, const escoin_solver_desc *desc, double *diff, double *history,
                               double *history2, double *dense_w);
ESCOIN_API int escoin_solver_array_step(const escoin_solver_desc *desc, long n, float *data, float *diff, float *history,
                             float *history2, void *stream);
ESCOIN_API int escoin_solver_array_step_f64(const escoin_solver_desc *desc, long n, double *data, double *diff,
                                 double *history, double *history2, void *stream);
ESCOIN_API int escoin_solver_array_step_cpu(const escoin_solver_desc *desc, long n, float *data, float *diff,
                                 float *history, float *history2);
ESCOIN_API int escoin_solver_array_step_cpu_f64(const escoin_solver_desc *desc, long n, double *data, double *diff,
                                     double *history, double *history2);

/* ---- Pruning: magnitude pruning of an aligned plan, in place, with the entry map that carries the solver state over ----
 * Gradual pruning is train, drop the smallest weights, train on.  Everything above keeps the pattern; this is the verb
 * that SHRINKS it, and it hands back what a caller needs to keep its compact arrays (history, history2, a pending
 * values_diff: nnz elements in escoin_plan_get_csr's order) in step: the old-entry -> new-entry map.
 * One entry point for both Dtypes: the plan knows its Dtype, and `score` is read as that type.
 * The rule, exact and the same on device and host:
 *   key(s) = the bits of s with the sign bit cleared, compared as an unsigned integer (float: 32 bits, double: 64).  No
 *   floating-point comparison is made anywhere: -0.0 == +0.0, denormals rank exactly, inf ranks above every finite value
 *   and NaN above inf (a NaN weight is never silently pruned away).
 *   KEEP orders the entries by (key descending, entry index ascending) over the whole layer, all conv groups together, and
 *   keeps the first min(keep, nnz): among equal keys the lower entry index stays.
 *   THRESHOLD keeps an entry iff key(s) >= key(threshold); the threshold is converted to the plan's Dtype once.
 *   Explicit zeros of the pattern are ordinary entries with key 0.
 *   score == NULL ranks the plan's current values; after a device-source update or solver step those are the DEVICE's, and
 *   the caller does not synchronise first: the plan orders itself behind the stream of that update, as the read-back does.
 * Effect: entry_map[e], e in [0, old nnz), is entry e's index in the new CSR, or -1 if it was dropped; the kept entries
 * keep their order, so the map ascends over them.  entry_map and new_nnz may each be NULL.  Afterwards every consumer of
 * the plan -- forward in all four conv_modes, backward, get_csr, export_aligned, updates, the solver step, the CPU entry
 * points -- behaves BIT FOR BIT like a fresh plan with the same options aligned by escoin_plan_set_csr on the kept entries:
 * the dense / sparse split, the kernel choice and the tiling are decided anew (sync_host_values, a new host CSR,
 * realign_from_host_csr); the backward state and the update state are dropped, as on any align.  Dropping every entry
 * leaves what escoin_plan_set_csr leaves on an empty CSR: an aligned plan with nnz 0 whose forward writes the bias (or 0).
 * When nothing is dropped (keep >= nnz, every key passes the threshold, nnz == 0) the plan is untouched: no re-align, the
 * states stay, the map is the identity, ESCOIN_OK, "prune_last_dropped" = 0.
 * The call synchronises (`stream`, and the last update's stream) and allocates: it is NOT CAPTURABLE.
 * Device side (prune_select.hip, on the kernels of radix_select.h that escoin_plan_rewire shares): a radix select of the
 * keep-th largest key, 8 bits a pass (select_hist_kernel: 4 histogram launches for float, 8 for double; the digit is chosen
 * on the device by select_choose_kernel, no host round trip between passes), then per-tile counts (select_count_kernel),
 * one workgroup's scan of the tile counts (select_scan_kernel) and the map (escoin_prune_apply_kernel) -- integer atomics
 * only, and no workgroup waits for another one.
 * escoin_plan_prune_cpu: the same rule as plain host code, for plans aligned by escoin_weight_align_cpu; no HIP call.
 * escoin_compact_entries: dst[entry_map[e]] = src[e] wherever entry_map[e] >= 0 -- what the caller runs over history,
 * history2, a pending values_diff or its own copy of the values.  dst holds the new nnz elements; src and dst must NOT
 * overlap (only an equal pointer is detected: ESCOIN_EINVAL).  dst == NULL is a destination of 0 elements (every entry was
 * dropped): nothing is stored or launched; the host route refuses it (ESCOIN_EINVAL) if the map keeps an entry.  on_device != 0: device pointers, one launch of
 * escoin_compact_kernel (one lane per old entry, one plain store), asynchronous on `stream`, capturable.  on_device == 0:
 * host pointers, a plain loop, no HIP call.
 * Errors: ESCOIN_EINVAL for a NULL desc, an unknown mode, keep < 0, a negative or NaN threshold, elem_bytes not 4 or 8,
 * old_nnz < 0; ESCOIN_ENODEVICE for the device entry points without a device; ESCOIN_ESTATE before an align, on another
 * device, for escoin_plan_prune_cpu on a device-aligned plan and for escoin_plan_prune on a CPU-aligned one.
 * Stats: "prune_count" (prunes since the plan was created), "prune_last_dropped" (entries the last prune dropped),
 * "prune_tile_entries" (the entries one workgroup of the count / map kernels covers per step: a constant of the build);
 * of the last escoin_plan_prune: "prune_kernels_us" (the selection, scan and map launches, by device events),
 * "prune_map_us" (the call's wall time until the host holds the map), "prune_realign_us" (from there to the end of the
 * re-align; 0 when nothing was dropped); "align_us" is then the whole call. */
#define ESCOIN_PRUNE_KEEP 0       /* keep exactly min(keep, nnz) entries: the largest |s| */
#define ESCOIN_PRUNE_THRESHOLD 1  /* keep the entries with |s| >= threshold */
typedef struct escoin_prune_desc {
  int mode;
  long keep;            /* KEEP */
  double threshold;     /* THRESHOLD; converted to the plan's Dtype once; >= 0, not NaN */
  const void *score;    /* NULL: s = the plan's current values.  Otherwise nnz elements of the plan's Dtype in
                           get_csr's order (device pointer; host pointer for _cpu), e.g. |w * g| */
} escoin_prune_desc;
ESCOIN_API int escoin_plan_prune(escoin_plan *plan, const escoin_prune_desc *desc, int *entry_map_dev, long *new_nnz,
                      void *stream);
ESCOIN_API int escoin_plan_prune_cpu(escoin_plan *plan, const escoin_prune_desc *desc, int *entry_map, long *new_nnz);
ESCOIN_API int escoin_compact_entries(const int *entry_map, long old_nnz, int elem_bytes /* 4 | 8 */, const void *src,
                           void *dst, int on_device, void *stream);

/* ---- Rewiring: drop and grow in one call, with one re-align, and the map that carries the solver state over ----
 * Dynamic sparse training (RigL, SET, any prune-and-regrow schedule) drops the k smallest weights and grows k positions
 * where a dense score -- usually the dense gradient's magnitude -- is largest.  escoin_plan_prune shrinks the pattern;
 * this is the verb that GROWS it, and it does both at once.
 * Notation: kdim = Cg * KH * KW, D = M * kdim; a position is p = oc * kdim + colidx with oc counted over all conv
 * groups, i.e. an element of blobs_[0]; ascending p over a pattern is escoin_plan_get_csr's order; P is the plan's
 * current pattern with nnz entries.  The rule, exact and the same on device and host:
 *   Drop (optional): `drop` is an escoin_prune_desc whose rule is exactly escoin_plan_prune's, over the plan's entries:
 *   KEEP or THRESHOLD, score NULL (the current values, the device's if it is authoritative) or a per-entry score.  It
 *   yields the kept set K, a subset of P; drop == NULL gives K = P.
 *   Grow: the candidates are the positions NOT in P.  A position this call drops is not a candidate in the same call, so
 *   the two selections are independent and each equals its stand-alone rule (a caller who wants to regrow a weight it
 *   just dropped calls escoin_plan_prune first).  key(s) is prune's key: the bits of s without the sign bit, as an
 *   unsigned integer; no floating-point comparison is made anywhere.  A NaN score ranks HIGHEST and is grown first; a zero
 *   score is an ordinary candidate.  The candidates are ordered by (key(score[p]) descending, p ascending) and the first
 *   n_grown = min(grow, D - nnz) are grown.  `score` is a dense array of D elements of the plan's Dtype, shaped like
 *   blobs_[0]; it is read only at candidate positions (a NaN inside the pattern does no harm).
 *   Result: the new pattern is K united with the grown set G, in ascending p.  Kept entries keep their value bits.  A
 *   grown entry is an explicit +0.0; with init != NULL it takes the bits of init[p] instead (init: a dense D-element
 *   array, read only at grown positions).  entry_map[e], e in [0, old nnz), is the entry's new index, or -1 if it was
 *   dropped.  grown[i], i in [0, n_grown), is the new entry index of the i-th grown position, in ascending position order
 *   (grown_dev holds `grow` ints; only the first n_grown are written).  entry_map, grown, new_nnz and n_grown may each be
 *   NULL.
 * Afterwards every consumer of the plan behaves BIT FOR BIT like a fresh plan with the same options aligned by
 * escoin_plan_set_csr on the new CSR, and only ONE re-align happened.  The backward state and the update state are
 * dropped, as on any align.  When nothing is dropped and nothing is grown (grow == 0 or no candidates, and no drop or a
 * drop that keeps everything) the plan is untouched and the map is the identity.  With grow == 0 the map and the plan equal
 * escoin_plan_prune's with the same descriptor, bit for bit.  An aligned plan with nnz 0 can be grown.
 * The call synchronises and allocates, like a prune: it is NOT CAPTURABLE.  It orders itself behind the last update's
 * stream, as a prune does.
 * Carrying momentum over -- the recipe.  The compact per-entry arrays (history, history2, a pending values_diff) move with
 * the existing escoin_compact_entries into a ZERO-FILLED array of the new nnz:
 *     new_h = zeros(new_nnz);  escoin_compact_entries(entry_map, old_nnz, elem_bytes, h, new_h, on_device, stream);
 * kept entries keep their history, grown entries (the indices in `grown`) start with zero momentum, and the next
 * escoin_solver_step runs on (new values_diff, new_h, new_h2) as if nothing had happened to the kept entries.
 * The dense score comes from the plan itself: escoin_dense_wgrad ("Dense weight gradient" below) writes the D-element
 * dense weight gradient that `score` reads, no abs needed.
 * Device side (rewire_select.hip): the drop is prune's launch sequence; over the D positions a mark launch (the host
 * CSR's entry positions -> an int per position: candidate, dropped, or the kept entry's index), a radix select over the
 * candidates' keys (one histogram launch per key byte, the digit chosen on the device), per-tile counts, one workgroup's
 * scan, one launch that writes entry_map through the entries' positions and one that writes grown and the grown
 * values -- integer atomics only, and no workgroup waits for another one.
 * escoin_plan_rewire_cpu: the same rule as plain host code (rewire_rules), for plans aligned by escoin_weight_align_cpu;
 * score, init, entry_map and grown are then host pointers; no HIP call.
 * Errors follow escoin_plan_prune's (ESCOIN_EINVAL for a NULL desc or a bad `drop`, ESCOIN_ENODEVICE, ESCOIN_ESTATE);
 * ESCOIN_EINVAL also for grow < 0, for score == NULL with grow > 0, and for D >= 2^31.
 * Stats: "rewire_count", "rewire_last_dropped", "rewire_last_grown"; of the last escoin_plan_rewire "rewire_kernels_us"
 * (every launch, the drop's included, by device events), "rewire_map_us" (the call's wall time until the host holds the
 * map and the grown list), "rewire_realign_us" (from there to the end of the re-align; 0 when the plan was left
 * untouched).  The "prune_*" stats are not touched by a rewire. */
typedef struct escoin_rewire_desc {
  const escoin_prune_desc *drop;  /* NULL: nothing dropped */
  long grow;                      /* >= 0 */
  const void *score;              /* D elements, plan's Dtype; device (host for _cpu); may be NULL iff grow == 0 */
  const void *init;               /* NULL: grown entries are +0.0 */
} escoin_rewire_desc;
ESCOIN_API int escoin_plan_rewire(escoin_plan *plan, const escoin_rewire_desc *desc, int *entry_map_dev, int *grown_dev,
                       long *new_nnz, long *n_grown, void *stream);
ESCOIN_API int escoin_plan_rewire_cpu(escoin_plan *plan, const escoin_rewire_desc *desc, int *entry_map, int *grown,
                           long *new_nnz, long *n_grown);

/* ---- Dense weight gradient: the grow score of a rewire, from the sparse plan itself ------------------------------------
 *   weight_gpu_gemm (base_conv_layer.cpp:877-889): the reference's weight gradient is dense.
 * Every weight-gradient path of escoin_backward writes the CSR positions only; a RigL step needs the gradient OUTSIDE the
 * pattern.  With G = top_diff (x [top > 0] on fuse_relu plans),
 *   dense_diff[oc*kdim + k] = sum over (n < n_images, oh, ow) of G[n][oc][oh][ow] x bottom at column k's tap (0 outside the
 *   image), for ALL D = M*kdim positions of blobs_[0], inside and outside the pattern -- exactly the array
 *   escoin_rewire_desc.score reads.
 * accumulate == 0 overwrites every element; accumulate != 0 adds the gradient with one rounding.  n_images == 0 writes
 * zeros (nothing when accumulating); images at or past n_images are never read.  The result depends on the plan's geometry
 * and fuse_relu only, not on the pattern or the values; the call still requires an aligned plan (ESCOIN_ESTATE before) on
 * the current device.  A RigL step is  escoin_dense_wgrad -> escoin_plan_rewire(score = dense_diff) ->
 * escoin_compact_entries.
 * Device: float plans within the MFMA weight-gradient kernel's index limits (N*OH*OW, M*Cg*KH*KW and Cg*H*W below 2^31; H,
 * W, pads and dilated kernel extents below 2^28; at most 65535 (group, 64-channel tile) pairs and column tiles); a double
 * plan or one outside the limits gets ESCOIN_EINVAL, and escoin_dense_wgrad_f64 always does ("no double kernel: use
 * escoin_dense_wgrad_cpu_f64").  escoin_dense_wgrad_mfma_kernel: one workgroup of four waves per (split of the pixel axis,
 * 64 output channels of a conv group, 64 columns) multiplies G[64 x pixels] by the im2col view of the bottom on the fp32
 * matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums), 32 pixels per LDS step -- the step loop of
 * escoin_sconv_wgrad_mfma_kernel -- over its whole span of 1024-pixel chunks with one accumulator set, and writes its tile
 * to a partial slab; escoin_dense_wgrad_sum_kernel then sums the splits ascending, one lane per position.  The split:
 * with tiles = group x M-tiles x column tiles and resident = 4 x CUs workgroups on the device at once, cutting the chunks
 * into S = ceil(chunks / span) spans costs max(1, (r + ceil(r)) / 2) x span with r = tiles x S / resident (rounds of resident
 * workgroups, a partly filled last round counting half of what it leaves empty, x the chunks each workgroup walks) + S / 512
 * (the sum's serial walk); the plan takes the cheapest span among those of at most four rounds (ties:
 * the fewest splits; S = 1 where none qualifies).  A layer with few tiles still fills the device, and the slab is S x D
 * floats -- at most about 16 x CUs tiles of 16 KB, whatever the batch (csrc/align_rules.h dwg_plan; what was measured:
 * profiles/grow_score_mi355x.md).  Spans without a live pixel are not launched.
 * Deterministic: the sum order is a function of the geometry, n_images, the device's CU count and option
 * "dense_wgrad_splits" only; no atomics, no workgroup waits for another.  Zeros are staged by select: a non-finite bottom
 * element reaches only the columns whose tap reads it, a non-finite G only its own row.
 * State: the first device call builds the column decode table and the slab (allocations, a synchronisation).  They are a
 * function of the descriptor alone, so weight_align, set_csr, prune and rewire KEEP them; only escoin_plan_destroy frees
 * them (a call that finds the plan aligned on another device builds them anew there).  Later calls allocate nothing and
 * synchronise nothing: capturable in a graph after escoin_forward and escoin_backward.
 * The _cpu twins: plain host loops on any plan with a host CSR, both Dtypes; every element's sum runs over its pixels
 * ascending, whatever n_threads (as in escoin_forward_cpu); n_images is not bounded by desc.N.
 * Errors: ESCOIN_EINVAL for a NULL top_diff, bottom or dense_diff, fuse_relu without top, n_images outside [0, desc.N]
 * (GPU) / < 0 (CPU); ESCOIN_ESTATE before an align, on another device, on the other Dtype's _cpu entry point.
 * Option "dense_wgrad_splits" (test option, before the align): 0 = the rule above, n = at most n splits.  Results stay
 * within the same error bound for any value (the low bits differ: another sum order).
 * Stats: "dwg_device_bytes" (the state's device memory: 0 until the first call; part of escoin_plan_workspace_bytes),
 * "dwg_splits" (splits of the full batch; 0 until the first call), "dwg_lds_bytes" (LDS of a workgroup; 0 until the
 * first call), "dwg_count" (device calls since the plan was created). */
ESCOIN_API int escoin_dense_wgrad(escoin_plan *plan, const float *bottom_dev, const float *top_dev, const float *top_diff_dev,
                       float *dense_diff_dev, int n_images, int accumulate, void *stream);
ESCOIN_API int escoin_dense_wgrad_f64(escoin_plan *plan, const double *bottom_dev, const double *top_dev,
                           const double *top_diff_dev, double *dense_diff_dev, int n_images, int accumulate, void *stream);
ESCOIN_API int escoin_dense_wgrad_cpu(escoin_plan *plan, const float *bottom, const float *top, const float *top_diff,
                           float *dense_diff, int n_images, int accumulate, int n_threads);
ESCOIN_API int escoin_dense_wgrad_cpu_f64(escoin_plan *plan, const double *bottom, const double *top, const double *top_diff,
                               double *dense_diff, int n_images, int accumulate, int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* ESCOIN_H_ */
