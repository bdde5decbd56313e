(* hvc.ml -- ctypes binding of include/hvc_jpeg.h (libhvc_jpeg.so, the MI355X block-transform path).
   UNCOMPILED: the build image has no OCaml toolchain; see README.md in this directory.
   Every [foreign] below names the C prototype it binds; argument order is the header's. *)
open Ctypes
open Foreign

type ctx = unit ptr

let ctx : ctx typ = ptr void

(* hvc_status -> the model's error style (decoder.ml:67, 92, 101, 136) *)
let strerror = foreign "hvc_strerror" (int @-> returning string)

let check what code =
  if code <> 0
  then Base.raise_s [%message "hvc" (what : string) (code : int) (strerror code : string)]
;;

let mem_host = 0
let mem_device = 1

(* int hvc_create(hvc_ctx **out, int device); void hvc_destroy(hvc_ctx *) *)
let create = foreign "hvc_create" (ptr ctx @-> int @-> returning int)
let destroy = foreign "hvc_destroy" (ctx @-> returning void)

let with_ctx ?(device = 0) f =
  let p = allocate ctx null in
  check "hvc_create" (create p device);
  Base.Exn.protect ~f:(fun () -> f !@p) ~finally:(fun () -> destroy !@p)
;;

(* typedef struct hvc_component { int blocks_w, blocks_h, qtab, reserved;
                                  size_t coef_offset, plane_offset, stride; } *)
module Component = struct
  type t

  let t : t structure typ = structure "hvc_component"
  let blocks_w = field t "blocks_w" int
  let blocks_h = field t "blocks_h" int
  let qtab = field t "qtab" int
  let reserved = field t "reserved" int
  let coef_offset = field t "coef_offset" size_t
  let plane_offset = field t "plane_offset" size_t
  let stride = field t "stride" size_t
  let () = seal t
end

(* typedef struct hvc_jpeg_component { int identifier, hscale, vscale, decoded_width, decoded_height,
                                       actual_width, actual_height, dc_table, ac_table; } *)
module Jpeg_component = struct
  type t

  let t : t structure typ = structure "hvc_jpeg_component"
  let identifier = field t "identifier" int
  let hscale = field t "hscale" int
  let vscale = field t "vscale" int
  let decoded_width = field t "decoded_width" int
  let decoded_height = field t "decoded_height" int
  let actual_width = field t "actual_width" int
  let actual_height = field t "actual_height" int
  let dc_table = field t "dc_table" int
  let ac_table = field t "ac_table" int
  let () = seal t
end

(* typedef struct hvc_jpeg_info { int width, height, n_comp, n_qtabs; hvc_jpeg_component comp[4];
     hvc_component layout[4]; uint16_t qtabs[4][64]; size_t coef_count, pixel_bytes, ecs_offset; } *)
module Jpeg_info = struct
  type t

  let t : t structure typ = structure "hvc_jpeg_info"
  let width = field t "width" int
  let height = field t "height" int
  let n_comp = field t "n_comp" int
  let n_qtabs = field t "n_qtabs" int
  let comp = field t "comp" (array 4 Jpeg_component.t)
  let layout = field t "layout" (array 4 Component.t)
  let qtabs = field t "qtabs" (array 256 uint16_t)
  let coef_count = field t "coef_count" size_t
  let pixel_bytes = field t "pixel_bytes" size_t
  let ecs_offset = field t "ecs_offset" size_t
  let () = seal t
end

(* int hvc_dequant_idct_recon(ctx, coefs, coef_plane_stride, qtab, blocks_w, blocks_h, n_planes,
                              plane, stride, plane_stride, where)            decoder.ml:142-149, 213-224; dct.ml:11-107 *)
let dequant_idct_recon =
  foreign
    "hvc_dequant_idct_recon"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> size_t @-> ptr uint16_t @-> int @-> int @-> int @-> ptr char @-> size_t
    @-> size_t @-> int @-> returning int)
;;

(* int hvc_decode_frames(ctx, coefs, coef_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames,
                         pixels, pixel_frame_stride, where) *)
let decode_frames =
  foreign
    "hvc_decode_frames"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int
    @-> ptr char @-> size_t @-> int @-> returning int)
;;

(* int hvc_decode_frames_yuv444(ctx, coefs, coef_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames,
                                width, height, frames, frame_stride, where)
   decoder.ml:403-420 + tools/src/planar_444.ml:82-131 fused into the block stage *)
let decode_frames_yuv444 =
  foreign
    "hvc_decode_frames_yuv444"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int @-> int
    @-> int @-> ptr char @-> size_t @-> int @-> returning int)
;;

(* int hvc_fdct_quant(ctx, plane, stride, plane_stride, qtab, blocks_w, blocks_h, n_planes, coefs,
                      coef_plane_stride, where)                               encoder.ml:81-108; dct.ml:109-196 *)
let fdct_quant =
  foreign
    "hvc_fdct_quant"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> size_t @-> size_t @-> ptr uint16_t @-> int @-> int @-> int @-> ptr int16_t
    @-> size_t @-> int @-> returning int)
;;

(* whole-file entry points (host C++ front / back end + the GPU block stage) *)
let jpeg_read_header =
  foreign "hvc_jpeg_read_header" (string @-> size_t @-> ptr Jpeg_info.t @-> returning int)
;;

(* int hvc_jpeg_decode(ctx, jpeg, n, info, pixels, pixel_cap)                 decoder.ml:422-427 minus the crop *)
let jpeg_decode =
  foreign
    "hvc_jpeg_decode"
    ~release_runtime_lock:true
    (ctx @-> string @-> size_t @-> ptr Jpeg_info.t @-> ptr char @-> size_t @-> returning int)
;;

(* int hvc_jpeg_get_yuv_frame(info, pixels, out, cap, out_len)               decoder.ml:403-420; Frame.of_planes' raises = HVC_E_BAD_JPEG *)
let jpeg_get_yuv_frame =
  foreign
    "hvc_jpeg_get_yuv_frame"
    (ptr Jpeg_info.t @-> ptr char @-> ptr char @-> size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_jpeg_get_cropped_planes(info, pixels, out, cap, out_len)          decoder.ml:399-413: crop of every plane *)
let jpeg_get_cropped_planes =
  foreign
    "hvc_jpeg_get_cropped_planes"
    (ptr Jpeg_info.t @-> ptr char @-> ptr char @-> size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_jpeg_encode(ctx, y, u, v, width, height, chroma, quality, out, cap, out_len)   encoder.ml:512-541 *)
let jpeg_encode =
  foreign
    "hvc_jpeg_encode"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> ptr char @-> ptr char @-> int @-> int @-> int @-> int @-> ptr char @-> size_t
    @-> ptr size_t @-> returning int)
;;

(* int hvc_quant_table(chroma_table, quality, out64)                         quant_tables.ml:139-147 *)
let quant_table = foreign "hvc_quant_table" (int @-> int @-> ptr uint16_t @-> returning int)

(* int hvc_compare_planes(a, b, n, max_difference, total_difference, square_error)   tools/src/ocompare.ml:6-47 *)
let compare_planes =
  foreign
    "hvc_compare_planes"
    (ptr char @-> ptr char @-> size_t @-> ptr int @-> ptr uint64_t @-> ptr uint64_t @-> returning int)
;;

(* int hvc_encode_frames(ctx, pixels, pixel_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames, coefs,
                         coef_frame_stride, where)                            encoder.ml:81-108 for a frame batch *)
let encode_frames =
  foreign
    "hvc_encode_frames"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int
    @-> ptr int16_t @-> size_t @-> int @-> returning int)
;;

(* int hvc_encode_frames_recon(ctx, pixels, pixel_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames, coefs,
                               coef_frame_stride, recon, error, where)
   Encoder.encode_block with ~compute_reconstruction_error:true: encoder.ml:110-125, 195-205 *)
let encode_frames_recon =
  foreign
    "hvc_encode_frames_recon"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int
    @-> ptr int16_t @-> size_t @-> ptr char @-> ptr char @-> int @-> returning int)
;;

(* int hvc_jpeg_entropy_decode(jpeg, n, info, coefs)                         decoder.ml:118-140, 143, 362-395 *)
let jpeg_entropy_decode =
  foreign
    "hvc_jpeg_entropy_decode"
    (string @-> size_t @-> ptr Jpeg_info.t @-> ptr int16_t @-> returning int)
;;

(* int hvc_jpeg_decode_yuv444(ctx, jpeg, n, info, frame, frame_cap)          decode_a_frame + Planar_444.of_420 *)
let jpeg_decode_yuv444 =
  foreign
    "hvc_jpeg_decode_yuv444"
    ~release_runtime_lock:true
    (ctx @-> string @-> size_t @-> ptr Jpeg_info.t @-> ptr char @-> size_t @-> returning int)
;;

(* typedef struct hvc_batch_stats { double wall_ms, entropy_ms_sum, h2d_ms_sum, kernel_ms_sum, d2h_ms_sum;
     int chunks, threads, frames_per_chunk; uint64_t coef_bytes; double host_prep_ms_sum; } *)
module Batch_stats = struct
  type t

  let t : t structure typ = structure "hvc_batch_stats"
  let wall_ms = field t "wall_ms" double
  let entropy_ms_sum = field t "entropy_ms_sum" double
  let h2d_ms_sum = field t "h2d_ms_sum" double
  let kernel_ms_sum = field t "kernel_ms_sum" double
  let d2h_ms_sum = field t "d2h_ms_sum" double
  let chunks = field t "chunks" int
  let threads = field t "threads" int
  let frames_per_chunk = field t "frames_per_chunk" int
  let coef_bytes = field t "coef_bytes" uint64_t
  let host_prep_ms_sum = field t "host_prep_ms_sum" double
  let () = seal t
end

(* int hvc_jpeg_decode_batch(ctx, jpegs, sizes, n_frames, threads, frames_per_chunk, pixels, pixel_frame_stride,
                             where, stats)                                    BASELINE config 3 *)
let jpeg_decode_batch =
  foreign
    "hvc_jpeg_decode_batch"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> int @-> ptr char @-> size_t @-> int
    @-> ptr Batch_stats.t @-> returning int)
;;

(* int hvc_jpeg_decode_batch_gpu(ctx, jpegs, sizes, n_frames, threads, frames_per_chunk, pixels,
                                 pixel_frame_stride, where, yuv444, stats) *)
let jpeg_decode_batch_gpu =
  foreign
    "hvc_jpeg_decode_batch_gpu"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> int @-> ptr char @-> size_t @-> int @-> int
    @-> ptr Batch_stats.t @-> returning int)
;;

(* int hvc_checksum_records(ctx, data, record_bytes, record_stride, n_records, sums, where)   K5 *)
let checksum_records =
  foreign
    "hvc_checksum_records"
    ~release_runtime_lock:true
    (ctx @-> ptr void @-> size_t @-> size_t @-> int @-> ptr uint64_t @-> int @-> returning int)
;;

(* int hvc_set_stream(ctx, hip_stream); int hvc_reset_stream(ctx); int hvc_synchronize(ctx) *)
let set_stream = foreign "hvc_set_stream" (ctx @-> ptr void @-> returning int)
let reset_stream = foreign "hvc_reset_stream" (ctx @-> returning int)
let synchronize = foreign "hvc_synchronize" ~release_runtime_lock:true (ctx @-> returning int)

(* ---- the rest of include/hvc_jpeg.h, so that the binding names every entry point ---- *)

(* const char *hvc_version(void); int hvc_last_hip_error(ctx) *)
let version = foreign "hvc_version" (void @-> returning string)
let last_hip_error = foreign "hvc_last_hip_error" (ctx @-> returning int)

(* host threads of the batch pipelines: int hvc_host_threads(ctx, alive, ever_started); int hvc_host_threads_probe(threads);
   int hvc_set_host_cpus(ctx, cpulist); int hvc_get_host_cpus(ctx, out, cap, n_cpus) *)
let host_threads = foreign "hvc_host_threads" (ctx @-> ptr int @-> ptr uint64_t @-> returning int)
let host_threads_probe = foreign "hvc_host_threads_probe" (int @-> returning int)
let set_host_cpus = foreign "hvc_set_host_cpus" (ctx @-> string @-> returning int)
let get_host_cpus = foreign "hvc_get_host_cpus" (ctx @-> ptr char @-> size_t @-> ptr int @-> returning int)

(* timers, profiling, kernel choice: int hvc_timer_begin(ctx); int hvc_timer_end(ctx, ms); int hvc_set_profiling(ctx, enabled);
   int hvc_last_kernel_ms(ctx, ms); int hvc_kernel_ms_history(ctx, ms, n); int hvc_set_decode_kernel(ctx, which);
   int hvc_last_wide_blocks(ctx, count) *)
let timer_begin = foreign "hvc_timer_begin" (ctx @-> returning int)
let timer_end = foreign "hvc_timer_end" ~release_runtime_lock:true (ctx @-> ptr float @-> returning int)
let set_profiling = foreign "hvc_set_profiling" (ctx @-> int @-> returning int)
let last_kernel_ms = foreign "hvc_last_kernel_ms" (ctx @-> ptr float @-> returning int)
let kernel_ms_history = foreign "hvc_kernel_ms_history" (ctx @-> ptr float @-> int @-> returning int)
let set_decode_kernel = foreign "hvc_set_decode_kernel" (ctx @-> int @-> returning int)
let last_wide_blocks = foreign "hvc_last_wide_blocks" (ctx @-> ptr uint64_t @-> returning int)

(* int hvc_upsample420(ctx, src, cw, ch, src_stride, dst, dst_stride, n_planes, src_plane_stride, dst_plane_stride, where)
   tools/src/planar_444.ml:82-103 *)
let upsample420 =
  foreign
    "hvc_upsample420"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> int @-> int @-> size_t @-> ptr char @-> size_t @-> int @-> size_t @-> size_t @-> int
    @-> returning int)
;;

(* the rest of `oyuv convert` (tools/src/oconv.ml), plane by plane like hvc_upsample420:
   int hvc_subsample420(ctx, src, sw, sh, src_stride, dst, dst_stride, n_planes, src_plane_stride, dst_plane_stride, where)
   tools/src/planar_444.ml:69-80, 105-116 *)
let subsample420 =
  foreign
    "hvc_subsample420"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> int @-> int @-> size_t @-> ptr char @-> size_t @-> int @-> size_t @-> size_t @-> int
    @-> returning int)
;;

(* int hvc_subsample422(...)   tools/src/planar_444.ml:18-23, 35-44 *)
let subsample422 =
  foreign
    "hvc_subsample422"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> int @-> int @-> size_t @-> ptr char @-> size_t @-> int @-> size_t @-> size_t @-> int
    @-> returning int)
;;

(* int hvc_upsample422(...)    tools/src/planar_444.ml:25-33, 55-67 *)
let upsample422 =
  foreign
    "hvc_upsample422"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> int @-> int @-> size_t @-> ptr char @-> size_t @-> int @-> size_t @-> size_t @-> int
    @-> returning int)
;;

(* int hvc_crop_planes(ctx, src, sw, sh, src_stride, x_pos, y_pos, dst, dw, dh, dst_stride, n_planes, src_plane_stride,
   dst_plane_stride, where)   tools/src/yuv.ml:42-62 *)
let crop_planes =
  foreign
    "hvc_crop_planes"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> int @-> int @-> size_t @-> int @-> int @-> ptr char @-> int @-> int @-> size_t @-> int
    @-> size_t @-> size_t @-> int @-> returning int)
;;

(* int hvc_yuv_frame_bytes(format, width, height, bytes)   tools/src/yuv_format.ml:21-53 *)
let yuv_frame_bytes = foreign "hvc_yuv_frame_bytes" (int @-> int @-> int @-> ptr size_t @-> returning int)

(* int hvc_yuv_convert(ctx, src, src_format, src_w, src_h, x_off, y_off, dst, dst_format, dst_w, dst_h, n_frames, where)
   tools/src/oconv.ml:111-133 *)
let yuv_convert =
  foreign
    "hvc_yuv_convert"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> int @-> int @-> int @-> int @-> int @-> ptr char @-> int @-> int @-> int @-> int @-> int
    @-> returning int)
;;

(* an extension beyond the model (off by default): restart intervals honoured
   int hvc_jpeg_entropy_decode_restart(jpeg, n, info, coefs);  int hvc_set_restart_markers(ctx, honour) *)
let jpeg_entropy_decode_restart =
  foreign
    "hvc_jpeg_entropy_decode_restart"
    ~release_runtime_lock:true
    (string @-> size_t @-> ptr Jpeg_info.t @-> ptr int16_t @-> returning int)
;;

let set_restart_markers = foreign "hvc_set_restart_markers" (ctx @-> int @-> returning int)

(* the block stage's arithmetic: 0 = the model (default), 1 = the Hardcaml RTL datapath, 3 = libjpeg's (islow + fancy upsampling)
   int hvc_set_arithmetic(ctx, arith);  int hvc_get_arithmetic(ctx, arith) *)
let set_arithmetic = foreign "hvc_set_arithmetic" (ctx @-> int @-> returning int)
let get_arithmetic = foreign "hvc_get_arithmetic" (ctx @-> ptr int @-> returning int)

(* int hvc_decode_frames_divergence(ctx, coefs, coef_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames,
                                    max_diff, diff_frame_stride, where): max |model - hardcaml| per block *)
let decode_frames_divergence =
  foreign
    "hvc_decode_frames_divergence"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int
    @-> ptr char @-> size_t @-> int @-> returning int)
;;

(* the encoder's arithmetic, independent of set_arithmetic: 0 = the model (default), 1 = the Hardcaml RTL DCT + quantiser
   int hvc_set_encode_arithmetic(ctx, arith);  int hvc_get_encode_arithmetic(ctx, arith) *)
let set_encode_arithmetic = foreign "hvc_set_encode_arithmetic" (ctx @-> int @-> returning int)
let get_encode_arithmetic = foreign "hvc_get_encode_arithmetic" (ctx @-> ptr int @-> returning int)
(* the encoder bit-exact to libjpeg-turbo, a setting of its own:
   int hvc_set_encode_libjpeg(ctx, on);  int hvc_get_encode_libjpeg(ctx, on) *)
let set_encode_libjpeg = foreign "hvc_set_encode_libjpeg" (ctx @-> int @-> returning int)
let get_encode_libjpeg = foreign "hvc_get_encode_libjpeg" (ctx @-> ptr int @-> returning int)

(* int hvc_encode_frames_divergence(ctx, pixels, pixel_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames,
                                    max_diff, diff_frame_stride, where): max |model - hardcaml| coefficient per block *)
let encode_frames_divergence =
  foreign
    "hvc_encode_frames_divergence"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int
    @-> ptr char @-> size_t @-> int @-> returning int)
;;

(* int hvc_jpeg_entropy_decode2(jpeg_a, n_a, info_a, coefs_a, status_a, jpeg_b, n_b, info_b, coefs_b, status_b):
   two files decoded in turn on the calling thread *)
let jpeg_entropy_decode2 =
  foreign
    "hvc_jpeg_entropy_decode2"
    ~release_runtime_lock:true
    (string @-> size_t @-> ptr Jpeg_info.t @-> ptr int16_t @-> ptr int @-> string @-> size_t @-> ptr Jpeg_info.t
    @-> ptr int16_t @-> ptr int @-> returning int)
;;

(* int hvc_jpeg_entropy_decode_gpu(ctx, jpegs, sizes, n_frames, coefs, coef_frame_stride, where, info, used_gpu) *)
let jpeg_entropy_decode_gpu =
  foreign
    "hvc_jpeg_entropy_decode_gpu"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> ptr int16_t @-> size_t @-> int @-> ptr Jpeg_info.t @-> ptr int
    @-> returning int)
;;

(* int hvc_jpeg_decode_batch_yuv444(ctx, jpegs, sizes, n_frames, threads, frames_per_chunk, frames, frame_stride, where, stats) *)
let jpeg_decode_batch_yuv444 =
  foreign
    "hvc_jpeg_decode_batch_yuv444"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> int @-> ptr char @-> size_t @-> int
    @-> ptr Batch_stats.t @-> returning int)
;;

(* the encoder's side: int hvc_jpeg_encoder_layout(width, height, chroma, quality, info); int hvc_jpeg_encoder_check(info);
   int hvc_jpeg_header(info, out, cap, len); int hvc_jpeg_entropy_encode(info, coefs, out, cap, out_len)
   encoder.ml:347-349, 371-418, 437-472, 127-193 *)
let jpeg_encoder_layout =
  foreign "hvc_jpeg_encoder_layout" (int @-> int @-> int @-> int @-> ptr Jpeg_info.t @-> returning int)
;;

let jpeg_encoder_check = foreign "hvc_jpeg_encoder_check" (ptr Jpeg_info.t @-> returning int)

let jpeg_header =
  foreign "hvc_jpeg_header" (ptr Jpeg_info.t @-> ptr char @-> size_t @-> ptr size_t @-> returning int)
;;

let jpeg_entropy_encode =
  foreign
    "hvc_jpeg_entropy_encode"
    ~release_runtime_lock:true
    (ptr Jpeg_info.t @-> ptr int16_t @-> ptr char @-> size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_huffman_encode_frames(ctx, info, coefs, coef_frame_stride, n_frames, out, out_cap, offsets, where):
   the GPU Huffman coder on device- or host-resident coefficient records *)
let huffman_encode_frames =
  foreign
    "hvc_huffman_encode_frames"
    ~release_runtime_lock:true
    (ctx @-> ptr Jpeg_info.t @-> ptr int16_t @-> size_t @-> int @-> ptr char @-> size_t @-> ptr uint64_t @-> int
    @-> returning int)
;;

(* int hvc_huffman_code_tables(ctx, table_set, where, codes272): the encoder back ends' code tables (diagnostic;
   Tables.Encoder.dc_table / ac_table, tables.ml:504-545) *)
let huffman_code_tables =
  foreign "hvc_huffman_code_tables" (ctx @-> int @-> int @-> ptr uint32_t @-> returning int)
;;

(* int hvc_jpeg_encode_batch(ctx, frames, n_frames, width, height, chroma, quality, threads, frames_per_chunk, jpegs, caps,
                             sizes, stats) and the same with the Huffman coder on the GPU      BASELINE config 5, files out *)
let jpeg_encode_batch =
  foreign
    "hvc_jpeg_encode_batch"
    ~release_runtime_lock:true
    (ctx @-> ptr (ptr char) @-> int @-> int @-> int @-> int @-> int @-> int @-> int @-> ptr (ptr char) @-> ptr size_t
    @-> ptr size_t @-> ptr Batch_stats.t @-> returning int)
;;

let jpeg_encode_batch_gpu =
  foreign
    "hvc_jpeg_encode_batch_gpu"
    ~release_runtime_lock:true
    (ctx @-> ptr (ptr char) @-> int @-> int @-> int @-> int @-> int @-> int @-> int @-> ptr (ptr char) @-> ptr size_t
    @-> ptr size_t @-> ptr Batch_stats.t @-> returning int)
;;

(* device memory for callers that keep records resident: int hvc_device_alloc(ctx, bytes, out); int hvc_device_free(ctx, p);
   int hvc_memcpy_h2d(ctx, dst, src, bytes); int hvc_memcpy_d2h(ctx, dst, src, bytes) *)
let device_alloc = foreign "hvc_device_alloc" (ctx @-> size_t @-> ptr (ptr void) @-> returning int)
let device_free = foreign "hvc_device_free" (ctx @-> ptr void @-> returning int)
let memcpy_h2d = foreign "hvc_memcpy_h2d" ~release_runtime_lock:true (ctx @-> ptr void @-> ptr void @-> size_t @-> returning int)
let memcpy_d2h = foreign "hvc_memcpy_d2h" ~release_runtime_lock:true (ctx @-> ptr void @-> ptr void @-> size_t @-> returning int)

(* ---- the asynchronous seam: pinned host memory and slots (include/hvc_jpeg.h, "The asynchronous seam") ----
   While the GPU works on the batch submitted to one slot, the caller -- this library's own sequential Huffman reader,
   decoder.ml:118-140 -- fills the pinned record of the next one.  [Decoder.decode_frames_gpu] is built on these. *)
let slots = 4 (* enum { HVC_SLOTS = 4 } *)

(* int hvc_host_alloc(ctx, bytes, out); int hvc_host_free(ctx, p): pinned memory (hipHostMalloc)
   int hvc_host_register(ctx, p, bytes); int hvc_host_unregister(ctx, p): the caller's own memory pinned in place -- whole
   pages only (posix_memalign'ed / mmap'ed memory; Bigarray.create's is malloc'ed: use [pinned_coefs] / [pinned_bytes]) *)
let host_alloc = foreign "hvc_host_alloc" (ctx @-> size_t @-> ptr (ptr void) @-> returning int)
let host_free = foreign "hvc_host_free" (ctx @-> ptr void @-> returning int)
let host_register = foreign "hvc_host_register" (ctx @-> ptr void @-> size_t @-> returning int)
let host_unregister = foreign "hvc_host_unregister" (ctx @-> ptr void @-> returning int)

(* int hvc_decode_frames_submit(ctx, slot, coefs, coef_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames, pixels,
                                pixel_frame_stride, pixels_where): hvc_decode_frames on host records, returns at once *)
let decode_frames_submit =
  foreign
    "hvc_decode_frames_submit"
    (ctx @-> int @-> ptr int16_t @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int
    @-> ptr char @-> size_t @-> int @-> returning int)
;;

(* int hvc_encode_frames_submit(ctx, slot, pixels, pixel_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames, coefs,
                                coef_frame_stride, coefs_where): the encoder mirror *)
let encode_frames_submit =
  foreign
    "hvc_encode_frames_submit"
    (ctx @-> int @-> ptr char @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int
    @-> ptr int16_t @-> size_t @-> int @-> returning int)
;;

(* int hvc_wait(ctx, slot): blocks (runtime lock released) until the slot's results are visible; int hvc_slot_query(ctx, slot, done) *)
let wait = foreign "hvc_wait" ~release_runtime_lock:true (ctx @-> int @-> returning int)
let slot_query = foreign "hvc_slot_query" (ctx @-> int @-> ptr int @-> returning int)

(* typedef struct hvc_slot_stats { double h2d_ms, kernel_ms, d2h_ms; uint64_t h2d_bytes, d2h_bytes; } *)
module Slot_stats = struct
  type t

  let t : t structure typ = structure "hvc_slot_stats"
  let h2d_ms = field t "h2d_ms" double
  let kernel_ms = field t "kernel_ms" double
  let d2h_ms = field t "d2h_ms" double
  let h2d_bytes = field t "h2d_bytes" uint64_t
  let d2h_bytes = field t "d2h_bytes" uint64_t
  let () = seal t
end

(* int hvc_slot_last_stats(ctx, slot, stats) *)
let slot_last_stats = foreign "hvc_slot_last_stats" (ctx @-> int @-> ptr Slot_stats.t @-> returning int)

(* The model's parametric fixed-point DCT (Dct.Fixed_point) and jpeg/bin/dct.ml's precision search *)
let dct_forward = 0
let dct_inverse = 1
let dct_round_trip = 2

module Dct_config = struct
  type t

  let t : t structure typ = structure "hvc_dct_config"
  let mode = field t "mode" int
  let fwd_rom_prec = field t "fwd_rom_prec" int
  let fwd_transpose_prec = field t "fwd_transpose_prec" int
  let inv_rom_prec = field t "inv_rom_prec" int
  let inv_transpose_prec = field t "inv_transpose_prec" int
  let () = seal t
end

module Dct_error = struct
  type t

  let t : t structure typ = structure "hvc_dct_error"
  let max_error = field t "max_error" double
  let worst_block = field t "worst_block" uint64_t
  let () = seal t
end

(* host only: int hvc_dct_rom(rom_prec, rom64); int hvc_dct_matrix(m64); int hvc_dct_blocks(seed, range, first, n, out) *)
let dct_rom = foreign "hvc_dct_rom" (int @-> ptr int32_t @-> returning int)
let dct_matrix = foreign "hvc_dct_matrix" (ptr double @-> returning int)
let dct_blocks = foreign "hvc_dct_blocks" (uint64_t @-> int @-> uint64_t @-> size_t @-> ptr int32_t @-> returning int)

(* int hvc_dct_fixed(ctx, direction, rom_prec, transpose_prec, in, out, n_blocks, where);
   int hvc_dct_reference(ctx, direction, in, out, n_blocks, where) *)
let dct_fixed =
  foreign
    "hvc_dct_fixed"
    ~release_runtime_lock:true
    (ctx @-> int @-> int @-> int @-> ptr int32_t @-> ptr int32_t @-> size_t @-> int @-> returning int)
;;

let dct_reference =
  foreign
    "hvc_dct_reference"
    ~release_runtime_lock:true
    (ctx @-> int @-> ptr int32_t @-> ptr double @-> size_t @-> int @-> returning int)
;;

(* int hvc_dct_error_search(ctx, cfg, n_cfg, seed, range, first_block, n_blocks, results) *)
let dct_error_search =
  foreign
    "hvc_dct_error_search"
    ~release_runtime_lock:true
    (ctx @-> ptr Dct_config.t @-> size_t @-> uint64_t @-> int @-> uint64_t @-> uint64_t @-> ptr Dct_error.t
    @-> returning int)
;;

(* Plane.t (common/src/plane.ml:4-9) is a Base_bigstring = (char, int8_unsigned_elt, c_layout) Array1:
   its data pointer is passed zero-copy.  (Needs [Plane.plane : t -> Base_bigstring.t] exposed.) *)
let plane_ptr (p : Hardcaml_video_common.Plane.t) =
  bigarray_start array1 (Hardcaml_video_common.Plane.plane p)
;;

type coefs = (int, Bigarray.int16_signed_elt, Bigarray.c_layout) Bigarray.Array1.t

let coefs_ptr (c : coefs) = bigarray_start array1 c

(* Pinned records as Bigarrays: [hvc_host_alloc]'s memory wrapped, not copied.  The Bigarray does not own it:
   [free_pinned] gives it back (after the last [wait] on a submission that used it). *)
let pinned_coefs (hvc : ctx) n : coefs =
  let p = allocate (ptr void) null in
  check "hvc_host_alloc" (host_alloc hvc (Unsigned.Size_t.of_int (2 * n)) p);
  bigarray_of_ptr array1 n Bigarray.int16_signed (from_voidp int16_t !@p)
;;

let pinned_bytes (hvc : ctx) n : Base_bigstring.t =
  let p = allocate (ptr void) null in
  check "hvc_host_alloc" (host_alloc hvc (Unsigned.Size_t.of_int n) p);
  bigarray_of_ptr array1 n Bigarray.char (from_voidp char !@p)
;;

let free_pinned_coefs (hvc : ctx) (c : coefs) =
  check "hvc_host_free" (host_free hvc (to_voidp (bigarray_start array1 c)))
;;

let free_pinned_bytes (hvc : ctx) (b : Base_bigstring.t) =
  check "hvc_host_free" (host_free hvc (to_voidp (bigarray_start array1 b)))
;;

(* Markers.Dqt.elements (zig-zag order) -> the uint16[64] the C side reads *)
let qtab_of_int_array (q : int array) =
  let a = CArray.make uint16_t 64 in
  Array.iteri (fun i v -> CArray.set a i (Unsigned.UInt16.of_int v)) q;
  a
;;

(* Per-file optimised Huffman tables (an extension: Annex K.2 tables fitted to each file).  A Huff_spec is one DHT body;
   arrays of four are ordered DC0, DC1, AC0, AC1. *)
module Huff_spec = struct
  type t

  let t : t structure typ = structure "hvc_huff_spec"
  let bits = field t "bits" (array 16 uint8_t)
  let vals = field t "vals" (array 256 uint8_t)
  let n_vals = field t "n_vals" uint16_t
  let pad = field t "pad" uint16_t
  let () = seal t
end

(* int hvc_set_huffman_tables(ctx, which);  int hvc_get_huffman_tables(ctx, which): 0 default, 1 optimised *)
let set_huffman_tables = foreign "hvc_set_huffman_tables" (ctx @-> int @-> returning int)
let get_huffman_tables = foreign "hvc_get_huffman_tables" (ctx @-> ptr int @-> returning int)

(* int hvc_huffman_spec_from_counts(counts[256], out): ITU-T T.81 Annex K.2 *)
let huffman_spec_from_counts =
  foreign "hvc_huffman_spec_from_counts" (ptr uint64_t @-> ptr Huff_spec.t @-> returning int)
;;

(* int hvc_huffman_optimal_tables(info, coefs, out[4]) *)
let huffman_optimal_tables =
  foreign
    "hvc_huffman_optimal_tables"
    ~release_runtime_lock:true
    (ptr Jpeg_info.t @-> ptr int16_t @-> ptr Huff_spec.t @-> returning int)
;;

(* int hvc_jpeg_header_tables(info, specs[4], out, cap, len) *)
let jpeg_header_tables =
  foreign
    "hvc_jpeg_header_tables"
    (ptr Jpeg_info.t @-> ptr Huff_spec.t @-> ptr char @-> size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_jpeg_entropy_encode_tables(info, specs[4], coefs, out, cap, out_len) *)
let jpeg_entropy_encode_tables =
  foreign
    "hvc_jpeg_entropy_encode_tables"
    ~release_runtime_lock:true
    (ptr Jpeg_info.t @-> ptr Huff_spec.t @-> ptr int16_t @-> ptr char @-> size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_huffman_encode_frames_optimised(ctx, info, coefs, coef_frame_stride, n_frames, out, out_cap, offsets, specs,
                                           where): hvc_huffman_encode_frames with each frame's own tables *)
let huffman_encode_frames_optimised =
  foreign
    "hvc_huffman_encode_frames_optimised"
    ~release_runtime_lock:true
    (ctx @-> ptr Jpeg_info.t @-> ptr int16_t @-> size_t @-> int @-> ptr char @-> size_t @-> ptr uint64_t
    @-> ptr Huff_spec.t @-> int @-> returning int)
;;

(* Restart intervals (DRI + RSTn) in the files written.
   int hvc_set_restart_interval(ctx, mcus);  int hvc_get_restart_interval(ctx, mcus): 0 off, 1 .. 65535 MCUs *)
let set_restart_interval = foreign "hvc_set_restart_interval" (ctx @-> int @-> returning int)
let get_restart_interval = foreign "hvc_get_restart_interval" (ctx @-> ptr int @-> returning int)

(* int hvc_jpeg_header_restart(info, specs[4] or null, restart_interval, out, cap, len) *)
let jpeg_header_restart =
  foreign
    "hvc_jpeg_header_restart"
    (ptr Jpeg_info.t @-> ptr Huff_spec.t @-> int @-> ptr char @-> size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_jpeg_entropy_encode_restart(info, specs[4] or null, restart_interval, coefs, out, cap, out_len) *)
let jpeg_entropy_encode_restart =
  foreign
    "hvc_jpeg_entropy_encode_restart"
    ~release_runtime_lock:true
    (ptr Jpeg_info.t @-> ptr Huff_spec.t @-> int @-> ptr int16_t @-> ptr char @-> size_t @-> ptr size_t
    @-> returning int)
;;

(* int hvc_huffman_optimal_tables_restart(info, coefs, restart_interval, out[4]) *)
let huffman_optimal_tables_restart =
  foreign
    "hvc_huffman_optimal_tables_restart"
    ~release_runtime_lock:true
    (ptr Jpeg_info.t @-> ptr int16_t @-> int @-> ptr Huff_spec.t @-> returning int)
;;

(* int hvc_huffman_encode_frames_restart(ctx, info, coefs, coef_frame_stride, n_frames, restart_interval, tables, out,
                                         out_cap, offsets, specs, where): tables 0 default (specs null), 1 optimised *)
let huffman_encode_frames_restart =
  foreign
    "hvc_huffman_encode_frames_restart"
    ~release_runtime_lock:true
    (ctx @-> ptr Jpeg_info.t @-> ptr int16_t @-> size_t @-> int @-> int @-> int @-> ptr char @-> size_t
    @-> ptr uint64_t @-> ptr Huff_spec.t @-> int @-> returning int)
;;

(* RGB (an extension: JFIF colour conversion fused with the chroma resampling; include/hvc_jpeg.h, RGB).
   sampling 420 | 422 | 444 | 400 (luma only); layout 0 interleaved ([H, W, 3]), 1 planar ([3, H, W]); strides of 0 = tight.
   int hvc_yuv_to_rgb(ctx, yuv, yuv_frame_stride, comps, sampling, width, height, chroma_w, chroma_h, n_frames, rgb,
                      rgb_row_stride, rgb_frame_stride, layout, where) *)
let yuv_to_rgb =
  foreign
    "hvc_yuv_to_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> size_t @-> ptr Component.t @-> int @-> int @-> int @-> int @-> int @-> int @-> ptr char
    @-> size_t @-> size_t @-> int @-> int @-> returning int)
;;

(* int hvc_rgb_to_yuv(ctx, rgb, rgb_row_stride, rgb_frame_stride, layout, width, height, sampling, n_frames, yuv,
                      yuv_frame_stride, comps, where) *)
let rgb_to_yuv =
  foreign
    "hvc_rgb_to_yuv"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> size_t @-> size_t @-> int @-> int @-> int @-> int @-> int @-> ptr char @-> size_t
    @-> ptr Component.t @-> int @-> returning int)
;;

(* int hvc_decode_frames_rgb(ctx, coefs, coef_frame_stride, qtabs, n_qtabs, comps, n_comp, sampling, n_frames, width,
                             height, rgb, rgb_row_stride, rgb_frame_stride, layout, where) *)
let decode_frames_rgb =
  foreign
    "hvc_decode_frames_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int @-> int @-> int
    @-> int @-> ptr char @-> size_t @-> size_t @-> int @-> int @-> returning int)
;;

(* int hvc_jpeg_decode_rgb(ctx, jpeg, n, info, rgb, rgb_cap, rgb_row_stride, layout) *)
let jpeg_decode_rgb =
  foreign
    "hvc_jpeg_decode_rgb"
    ~release_runtime_lock:true
    (ctx @-> string @-> size_t @-> ptr Jpeg_info.t @-> ptr char @-> size_t @-> size_t @-> int @-> returning int)
;;

(* int hvc_jpeg_decode_batch_rgb(ctx, jpegs, sizes, n_frames, threads, frames_per_chunk, gpu_reader, rgb, rgb_row_stride,
                                 rgb_frame_stride, layout, where, stats) *)
let jpeg_decode_batch_rgb =
  foreign
    "hvc_jpeg_decode_batch_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> int @-> int @-> ptr char @-> size_t @-> size_t @-> int
    @-> int @-> ptr Batch_stats.t @-> returning int)
;;

(* Decoding at 1/2, 1/4, 1/8 size (include/hvc_jpeg.h, "Decoding at reduced size"): scale_denom = 1 | 2 | 4 | 8.
   int hvc_jpeg_scaled_info(info, scale_denom, out)                                                          host only *)
let jpeg_scaled_info =
  foreign "hvc_jpeg_scaled_info" (ptr Jpeg_info.t @-> int @-> ptr Jpeg_info.t @-> returning int)
;;

(* int hvc_decode_frames_scaled(ctx, coefs, coef_frame_stride, qtabs, n_qtabs, comps, n_comp, n_frames, scale_denom, pixels,
                                pixel_frame_stride, where) *)
let decode_frames_scaled =
  foreign
    "hvc_decode_frames_scaled"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> size_t @-> ptr uint16_t @-> int @-> ptr Component.t @-> int @-> int @-> int
    @-> ptr char @-> size_t @-> int @-> returning int)
;;

(* int hvc_jpeg_decode_scaled(ctx, jpeg, n, scale_denom, info, pixels, pixel_cap) *)
let jpeg_decode_scaled =
  foreign
    "hvc_jpeg_decode_scaled"
    ~release_runtime_lock:true
    (ctx @-> string @-> size_t @-> int @-> ptr Jpeg_info.t @-> ptr char @-> size_t @-> returning int)
;;

(* int hvc_jpeg_decode_scaled_rgb(ctx, jpeg, n, scale_denom, info, rgb, rgb_cap, rgb_row_stride, layout) *)
let jpeg_decode_scaled_rgb =
  foreign
    "hvc_jpeg_decode_scaled_rgb"
    ~release_runtime_lock:true
    (ctx @-> string @-> size_t @-> int @-> ptr Jpeg_info.t @-> ptr char @-> size_t @-> size_t @-> int @-> returning int)
;;

(* int hvc_jpeg_decode_batch_scaled(ctx, jpegs, sizes, n_frames, threads, frames_per_chunk, gpu_reader, scale_denom, pixels,
                                    pixel_frame_stride, where, stats) *)
let jpeg_decode_batch_scaled =
  foreign
    "hvc_jpeg_decode_batch_scaled"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> int @-> int @-> int @-> ptr char @-> size_t @-> int
    @-> ptr Batch_stats.t @-> returning int)
;;

(* Mixed batches (include/hvc_jpeg.h, "Mixed batches"): files and frames of different geometry and tables in one call.
   int hvc_jpeg_mixed_layout(jpegs, sizes, n_files, align, infos, status, pixel_offsets, total_bytes)          host only *)
let jpeg_mixed_layout =
  foreign
    "hvc_jpeg_mixed_layout"
    (ptr string @-> ptr size_t @-> int @-> size_t @-> ptr Jpeg_info.t @-> ptr int @-> ptr size_t @-> ptr size_t
    @-> returning int)
;;

(* int hvc_decode_frames_mixed(ctx, coefs, coef_offsets, infos, n_frames, pixels, pixel_offsets, where) *)
let decode_frames_mixed =
  foreign
    "hvc_decode_frames_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> ptr size_t @-> ptr Jpeg_info.t @-> int @-> ptr char @-> ptr size_t @-> int
    @-> returning int)
;;

(* int hvc_jpeg_decode_batch_mixed(ctx, jpegs, sizes, n_files, threads, chunk_bytes, infos, status, pixel_offsets, pixels,
                                   pixel_cap, where, stats) *)
let jpeg_decode_batch_mixed =
  foreign
    "hvc_jpeg_decode_batch_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> size_t @-> ptr Jpeg_info.t @-> ptr int @-> ptr size_t
    @-> ptr char @-> size_t @-> int @-> ptr Batch_stats.t @-> returning int)
;;

(* who reads the files of the mixed batch calls: 0 = HVC_READER_HOST (default), 1 = HVC_READER_GPU (the mixed GPU Huffman reader).
   int hvc_set_mixed_reader(ctx, which);  int hvc_get_mixed_reader(ctx, which);
   int hvc_last_mixed_reader_files(ctx, gpu_files, host_files) *)
let set_mixed_reader = foreign "hvc_set_mixed_reader" (ctx @-> int @-> returning int)
let get_mixed_reader = foreign "hvc_get_mixed_reader" (ctx @-> ptr int @-> returning int)

let last_mixed_reader_files =
  foreign "hvc_last_mixed_reader_files" (ctx @-> ptr uint64_t @-> ptr uint64_t @-> returning int)
;;

(* the mixed decode calls' own arithmetic: 0 = the model (default), 3 = libjpeg's (k_islow_mixed + k_ycc_to_rgb_fancy_mixed);
   under 3 they do not look at set_arithmetic, and the reduced-size forms are refused
   int hvc_set_mixed_arithmetic(ctx, arith);  int hvc_get_mixed_arithmetic(ctx, arith) *)
let set_mixed_arithmetic = foreign "hvc_set_mixed_arithmetic" (ctx @-> int @-> returning int)
let get_mixed_arithmetic = foreign "hvc_get_mixed_arithmetic" (ctx @-> ptr int @-> returning int)

(* int hvc_jpeg_entropy_decode_gpu_mixed(ctx, jpegs, sizes, n_files, infos, status, coefs, coef_offsets, coef_cap, where,
                                         used_gpu) *)
let jpeg_entropy_decode_gpu_mixed =
  foreign
    "hvc_jpeg_entropy_decode_gpu_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> ptr Jpeg_info.t @-> ptr int @-> ptr int16_t @-> ptr size_t @-> size_t
    @-> int @-> ptr int @-> returning int)
;;

(* mixed batches to RGB: one launch of the colour pass over images of any size and sampling.
   int hvc_jpeg_mixed_rgb_layout(jpegs, sizes, n_files, layout, align, row_align, infos, status, rgb_offsets,
                                 rgb_row_strides, total_bytes)                                                  host only *)
let jpeg_mixed_rgb_layout =
  foreign
    "hvc_jpeg_mixed_rgb_layout"
    (ptr string @-> ptr size_t @-> int @-> int @-> size_t @-> size_t @-> ptr Jpeg_info.t @-> ptr int @-> ptr size_t
    @-> ptr size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_yuv_to_rgb_mixed(ctx, yuv, yuv_offsets, infos, n_frames, rgb, rgb_offsets, rgb_row_strides, layout, where) *)
let yuv_to_rgb_mixed =
  foreign
    "hvc_yuv_to_rgb_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> ptr size_t @-> ptr Jpeg_info.t @-> int @-> ptr char @-> ptr size_t @-> ptr size_t @-> int
    @-> int @-> returning int)
;;

(* int hvc_decode_frames_mixed_rgb(ctx, coefs, coef_offsets, infos, n_frames, rgb, rgb_offsets, rgb_row_strides, layout,
                                   where) *)
let decode_frames_mixed_rgb =
  foreign
    "hvc_decode_frames_mixed_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> ptr size_t @-> ptr Jpeg_info.t @-> int @-> ptr char @-> ptr size_t @-> ptr size_t @-> int
    @-> int @-> returning int)
;;

(* int hvc_jpeg_decode_batch_mixed_rgb(ctx, jpegs, sizes, n_files, threads, chunk_bytes, infos, status, rgb_offsets,
                                       rgb_row_strides, rgb, rgb_cap, layout, where, stats) *)
let jpeg_decode_batch_mixed_rgb =
  foreign
    "hvc_jpeg_decode_batch_mixed_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> size_t @-> ptr Jpeg_info.t @-> ptr int @-> ptr size_t
    @-> ptr size_t @-> ptr char @-> size_t @-> int @-> int @-> ptr Batch_stats.t @-> returning int)
;;

(* mixed batches at 1/2, 1/4, 1/8 size (scale_denom 1 = the full-size call of the same name without "_scaled").
   int hvc_jpeg_mixed_scaled_layout(jpegs, sizes, n_files, scale_denom, align, infos, scaled, status, pixel_offsets,
                                    total_bytes)                                                                host only *)
let jpeg_mixed_scaled_layout =
  foreign
    "hvc_jpeg_mixed_scaled_layout"
    (ptr string @-> ptr size_t @-> int @-> int @-> size_t @-> ptr Jpeg_info.t @-> ptr Jpeg_info.t @-> ptr int
    @-> ptr size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_decode_frames_mixed_scaled(ctx, coefs, coef_offsets, infos, n_frames, scale_denom, pixels, pixel_offsets, where) *)
let decode_frames_mixed_scaled =
  foreign
    "hvc_decode_frames_mixed_scaled"
    ~release_runtime_lock:true
    (ctx @-> ptr int16_t @-> ptr size_t @-> ptr Jpeg_info.t @-> int @-> int @-> ptr char @-> ptr size_t @-> int
    @-> returning int)
;;

(* int hvc_jpeg_decode_batch_mixed_scaled(ctx, jpegs, sizes, n_files, threads, chunk_bytes, scale_denom, infos, status,
                                          pixel_offsets, pixels, pixel_cap, where, stats) *)
let jpeg_decode_batch_mixed_scaled =
  foreign
    "hvc_jpeg_decode_batch_mixed_scaled"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> size_t @-> int @-> ptr Jpeg_info.t @-> ptr int @-> ptr size_t
    @-> ptr char @-> size_t @-> int @-> ptr Batch_stats.t @-> returning int)
;;

(* int hvc_jpeg_mixed_scaled_rgb_layout(jpegs, sizes, n_files, scale_denom, layout, align, row_align, infos, scaled, status,
                                        rgb_offsets, rgb_row_strides, total_bytes)                              host only *)
let jpeg_mixed_scaled_rgb_layout =
  foreign
    "hvc_jpeg_mixed_scaled_rgb_layout"
    (ptr string @-> ptr size_t @-> int @-> int @-> int @-> size_t @-> size_t @-> ptr Jpeg_info.t @-> ptr Jpeg_info.t
    @-> ptr int @-> ptr size_t @-> ptr size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_jpeg_decode_batch_mixed_scaled_rgb(ctx, jpegs, sizes, n_files, threads, chunk_bytes, scale_denom, infos, status,
                                              rgb_offsets, rgb_row_strides, rgb, rgb_cap, layout, where, stats) *)
let jpeg_decode_batch_mixed_scaled_rgb =
  foreign
    "hvc_jpeg_decode_batch_mixed_scaled_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> size_t @-> int @-> ptr Jpeg_info.t @-> ptr int @-> ptr size_t
    @-> ptr size_t @-> ptr char @-> size_t @-> int @-> int @-> ptr Batch_stats.t @-> returning int)
;;

(* resizing a mixed set (bit-exact to Pillow's Image.resize; filter: 0 box, 1 bilinear, 2 bicubic).
   int hvc_rgb_resize_mixed(ctx, src, src_offsets, src_row_strides, widths, heights, n_images, dst, dst_offsets,
                            dst_row_strides, out_widths, out_heights, layout, filter, where) *)
let rgb_resize_mixed =
  foreign
    "hvc_rgb_resize_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> ptr size_t @-> ptr size_t @-> ptr int @-> ptr int @-> int @-> ptr char @-> ptr size_t
    @-> ptr size_t @-> ptr int @-> ptr int @-> int @-> int @-> int @-> returning int)
;;

(* int hvc_jpeg_decode_batch_mixed_resized(ctx, jpegs, sizes, n_files, threads, chunk_bytes, scale_denom, infos, status,
                                           out_widths, out_heights, dst_offsets, dst_row_strides, dst, dst_cap, layout,
                                           filter, where, stats) *)
let jpeg_decode_batch_mixed_resized =
  foreign
    "hvc_jpeg_decode_batch_mixed_resized"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> size_t @-> int @-> ptr Jpeg_info.t @-> ptr int @-> ptr int
    @-> ptr int @-> ptr size_t @-> ptr size_t @-> ptr char @-> size_t @-> int @-> int @-> int @-> ptr Batch_stats.t
    @-> returning int)
;;

(* the option block of the resizing calls: a box (4 singles: x0, y0, x1, y1) and a mirror flag per image, and a typed output
   looked up in a host table of 3 * 256 elements of out_elem bytes (0: 8-bit samples).  A null pointer or an all-zero block is
   the call without it.
   typedef struct hvc_resize_opts { const float *boxes; const uint8_t *mirror; int out_elem; const void *lut; } *)
module Resize_opts = struct
  type t

  let t : t structure typ = structure "hvc_resize_opts"
  let boxes = field t "boxes" (ptr float)
  let mirror = field t "mirror" (ptr uint8_t)
  let out_elem = field t "out_elem" int
  let lut = field t "lut" (ptr void)
  let () = seal t
end

(* int hvc_rgb_resize_mixed_opts(... hvc_rgb_resize_mixed's arguments ..., opts) *)
let rgb_resize_mixed_opts =
  foreign
    "hvc_rgb_resize_mixed_opts"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> ptr size_t @-> ptr size_t @-> ptr int @-> ptr int @-> int @-> ptr char @-> ptr size_t
    @-> ptr size_t @-> ptr int @-> ptr int @-> int @-> int @-> int @-> ptr Resize_opts.t @-> returning int)
;;

(* int hvc_jpeg_decode_batch_mixed_resized_opts(... hvc_jpeg_decode_batch_mixed_resized's arguments ..., opts) *)
let jpeg_decode_batch_mixed_resized_opts =
  foreign
    "hvc_jpeg_decode_batch_mixed_resized_opts"
    ~release_runtime_lock:true
    (ctx @-> ptr string @-> ptr size_t @-> int @-> int @-> size_t @-> int @-> ptr Jpeg_info.t @-> ptr int @-> ptr int
    @-> ptr int @-> ptr size_t @-> ptr size_t @-> ptr char @-> size_t @-> int @-> int @-> int @-> ptr Batch_stats.t
    @-> ptr Resize_opts.t @-> returning int)
;;

(* host only: int hvc_normalize_lut(mean, std, elem, lut): elem 1 float32, 2 float16, 3 bfloat16; lut: 3 * 256 elements *)
let normalize_lut = foreign "hvc_normalize_lut" (ptr float @-> ptr float @-> int @-> ptr void @-> returning int)

(* mixed batches, encoding: frames of different sizes, samplings and qualities in one call.
   int hvc_jpeg_encoder_mixed_layout(widths, heights, chromas, qualities, n_frames, align, infos, status, pixel_offsets,
                                     coef_offsets, pixel_total, coef_total)                                     host only *)
let jpeg_encoder_mixed_layout =
  foreign
    "hvc_jpeg_encoder_mixed_layout"
    (ptr int @-> ptr int @-> ptr int @-> ptr int @-> int @-> size_t @-> ptr Jpeg_info.t @-> ptr int @-> ptr size_t
    @-> ptr size_t @-> ptr size_t @-> ptr size_t @-> returning int)
;;

(* int hvc_encode_frames_mixed(ctx, pixels, pixel_offsets, infos, n_frames, coefs, coef_offsets, where) *)
let encode_frames_mixed =
  foreign
    "hvc_encode_frames_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> ptr size_t @-> ptr Jpeg_info.t @-> int @-> ptr int16_t @-> ptr size_t @-> int
    @-> returning int)
;;

(* int hvc_jpeg_encode_batch_mixed(ctx, frames, infos, status, n_frames, threads, chunk_bytes, jpegs, caps, sizes, stats) *)
let jpeg_encode_batch_mixed =
  foreign
    "hvc_jpeg_encode_batch_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr (ptr char) @-> ptr Jpeg_info.t @-> ptr int @-> int @-> int @-> size_t @-> ptr (ptr char) @-> ptr size_t
    @-> ptr size_t @-> ptr Batch_stats.t @-> returning int)
;;

(* mixed batches, encoding, with the Huffman coder on the GPU.
   int hvc_huffman_encode_frames_mixed(ctx, infos, coefs, coef_offsets, n_frames, tables, out, out_cap, offsets, status,
                                       specs, where): the coder alone, a status and a segment per frame *)
let huffman_encode_frames_mixed =
  foreign
    "hvc_huffman_encode_frames_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr Jpeg_info.t @-> ptr int16_t @-> ptr size_t @-> int @-> int @-> ptr char @-> size_t @-> ptr uint64_t
    @-> ptr int @-> ptr Huff_spec.t @-> int @-> returning int)
;;

(* int hvc_jpeg_encode_batch_mixed_gpu(ctx, frames, infos, status, n_frames, threads, chunk_bytes, jpegs, caps, sizes, stats) *)
let jpeg_encode_batch_mixed_gpu =
  foreign
    "hvc_jpeg_encode_batch_mixed_gpu"
    ~release_runtime_lock:true
    (ctx @-> ptr (ptr char) @-> ptr Jpeg_info.t @-> ptr int @-> int @-> int @-> size_t @-> ptr (ptr char) @-> ptr size_t
    @-> ptr size_t @-> ptr Batch_stats.t @-> returning int)
;;

(* int hvc_last_mixed_coder_files(ctx, gpu_files, host_files) *)
let last_mixed_coder_files =
  foreign "hvc_last_mixed_coder_files" (ctx @-> ptr uint64_t @-> ptr uint64_t @-> returning int)
;;

(* mixed batches, encoding, from RGB images.
   int hvc_jpeg_encoder_mixed_rgb_layout(widths, heights, chromas, qualities, n_frames, layout, align, row_align, infos, status,
                                         rgb_offsets, rgb_row_strides, rgb_total, pixel_offsets, coef_offsets, pixel_total,
                                         coef_total)                                                            host only *)
let jpeg_encoder_mixed_rgb_layout =
  foreign
    "hvc_jpeg_encoder_mixed_rgb_layout"
    (ptr int @-> ptr int @-> ptr int @-> ptr int @-> int @-> int @-> size_t @-> size_t @-> ptr Jpeg_info.t @-> ptr int
    @-> ptr size_t @-> ptr size_t @-> ptr size_t @-> ptr size_t @-> ptr size_t @-> ptr size_t @-> ptr size_t
    @-> returning int)
;;

(* int hvc_rgb_to_yuv_mixed(ctx, yuv, yuv_offsets, infos, n_frames, rgb, rgb_offsets, rgb_row_strides, layout, where) *)
let rgb_to_yuv_mixed =
  foreign
    "hvc_rgb_to_yuv_mixed"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> ptr size_t @-> ptr Jpeg_info.t @-> int @-> ptr char @-> ptr size_t @-> ptr size_t @-> int
    @-> int @-> returning int)
;;

(* int hvc_encode_frames_mixed_rgb(ctx, rgb, rgb_offsets, rgb_row_strides, layout, infos, n_frames, coefs, coef_offsets,
                                   where) *)
let encode_frames_mixed_rgb =
  foreign
    "hvc_encode_frames_mixed_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> ptr size_t @-> ptr size_t @-> int @-> ptr Jpeg_info.t @-> int @-> ptr int16_t @-> ptr size_t
    @-> int @-> returning int)
;;

(* int hvc_jpeg_encode_batch_mixed_rgb(ctx, frames, rgb_row_strides, layout, infos, status, n_frames, threads, chunk_bytes,
                                       jpegs, caps, sizes, stats) *)
let jpeg_encode_batch_mixed_rgb =
  foreign
    "hvc_jpeg_encode_batch_mixed_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr (ptr char) @-> ptr size_t @-> int @-> ptr Jpeg_info.t @-> ptr int @-> int @-> int @-> size_t
    @-> ptr (ptr char) @-> ptr size_t @-> ptr size_t @-> ptr Batch_stats.t @-> returning int)
;;

(* int hvc_jpeg_encode_batch_mixed_rgb_gpu(ctx, frames, rgb_row_strides, layout, infos, status, n_frames, threads, chunk_bytes,
                                           jpegs, caps, sizes, stats) *)
let jpeg_encode_batch_mixed_rgb_gpu =
  foreign
    "hvc_jpeg_encode_batch_mixed_rgb_gpu"
    ~release_runtime_lock:true
    (ctx @-> ptr (ptr char) @-> ptr size_t @-> int @-> ptr Jpeg_info.t @-> ptr int @-> int @-> int @-> size_t
    @-> ptr (ptr char) @-> ptr size_t @-> ptr size_t @-> ptr Batch_stats.t @-> returning int)
;;

(* int hvc_jpeg_encode_rgb(ctx, rgb, rgb_row_stride, layout, width, height, chroma, quality, out, cap, out_len) *)
let jpeg_encode_rgb =
  foreign
    "hvc_jpeg_encode_rgb"
    ~release_runtime_lock:true
    (ctx @-> ptr char @-> size_t @-> int @-> int @-> int @-> int @-> int @-> ptr char @-> size_t @-> ptr size_t
    @-> returning int)
;;
