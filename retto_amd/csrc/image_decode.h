// Encoded page -> RGB8: replaces ImageHelper::new_from_raw_img_flow
// (/root/reference/retto-core/src/image_helper.rs:34-44 = image::load_from_memory(bytes)?.to_rgb8()).
// Host code, like the reference's: the decoders are lossless-format readers written here (PNG over zlib's
// inflate, binary / ASCII PNM, uncompressed BMP) plus a Huffman-DCT JPEG reader
// (sequential and progressive).  Conversion to RGB8 follows the `image`
// crate 0.25.6 rules the reference relies on: alpha is dropped (not blended), grey is replicated,
// 16-bit samples map to 8 bits as (v + 128) / 257, sub-byte grey is scaled to the full range,
// palettes are expanded, gamma / colour-profile chunks are ignored.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rt {

// Throws RtError(RT_ERR_IMAGE) with the reason (unknown format, truncated stream, CRC mismatch, ...).
void decode_image(const uint8_t* data, size_t len, std::vector<uint8_t>* rgb, int* h, int* w);

// A JPEG page after entropy decoding, before any pixel work (the input of jpeg_kernels.hip).  Per component: sampling factors,
// real sample size (cw x ch), the MCU-padded plane (stride x rows), the quantisation table in natural order and the QUANTISED
// coefficients, 64 per 8x8 block in block raster order over the padded plane, natural order inside a block.
struct JpegCoefs {
  int W = 0, H = 0, nc = 0, hmax = 1, vmax = 1;
  bool is_rgb = false;   // three components coded as R, G, B (Adobe transform 0, or component ids 'R' 'G' 'B')
  struct Comp {
    int hs = 1, vs = 1, cw = 0, ch = 0, stride = 0, rows = 0;
    uint16_t q[64];
    std::vector<int16_t> coef;
  } c[3];
};
// One encoded page for the device path.  on_device: a JPEG whose pixels the kernels reconstruct from `jpeg` -- every quantised
// coefficient fits int16 and its sampling layout is one jpeg::layout_on_device accepts.  Otherwise `rgb` holds the page as
// decode_image decodes it (any other JPEG, PNG, PNM, BMP).  Errors are decode_image's.
struct EncodedPage {
  int h = 0, w = 0;
  bool on_device = false;
  JpegCoefs jpeg;
  std::vector<uint8_t> rgb;
};
void decode_for_device(const uint8_t* data, size_t len, EncodedPage* out);
// k_jpeg_idct + k_jpeg_color's arithmetic (jpeg_recon.h) run on the CPU: the RGB8 page the kernels produce from J
void reconstruct_host(const JpegCoefs& J, std::vector<uint8_t>* rgb);
// Page size from the header alone (no pixel work): RT_ERR_IMAGE for an unknown format or a bad header.
void image_dims(const uint8_t* data, size_t len, int* h, int* w);

}  // namespace rt
