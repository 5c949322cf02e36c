// vit_rs.hip -- Reed-Solomon decoding of the C ABI: vit_hip_rs_create / vit_hip_rs_destroy (a code over GF(256): the parameter rule,
// the tables built on the host by rs_tables.hpp and uploaded once) and vit_hip_rs_decode_batch (bounded-distance decoding of the
// interleaved codewords of frames in the layout vit_hip_frames_extract writes).  It works on the caller's bytes alone and reads the
// handle only for its device.  The kernel of kernels_rs.hpp is launched only here.  Host-side logic only: argument checking, the
// tables and the launch.
// Out of scope: erasure decoding; a GPU Reed-Solomon encoder; symbol sizes other than 8 bits.  DVB-S's Forney (12 x 17) convolutional
// de-interleaver and its inverted every-eighth sync byte live in vit_dvb.hip.
#include "vit_internal.hpp"
#include "kernels_rs.hpp"

using namespace vit;

struct vit_hip_rs_code_s {
    vit_hip_rs_params params;
    int device;
    uint8_t* d_tables;
};

namespace {

// argument rule (include/vit_hip.h): everything the host can know without reading device memory
const char* rs_decode_invalid(vit_hip_handle h, vit_hip_rs_code code, const uint8_t* d_in, const uint8_t* d_out, size_t stride, size_t rows,
                              size_t max_frames, size_t I, const int32_t* d_status) {
    if (!h || !code || !d_in || !d_out || !d_status) return "NULL handle, code or buffer";
    if (code->device != h->device) return "the code was made for another device";
    if (I == 0 || I > 0xFFFFFFu) return "interleave must be 1 .. 2^24 - 1";
    const size_t n = 255 - code->params.pad, frame = n * I;
    if (stride != 0 && stride < frame) return "frame_stride_bytes is below n * interleave";
    const size_t frames = rows * max_frames;
    if (frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu || frames * ((I + RS_TILE - 1) / RS_TILE) > 0x7FFFFFFFu)
        return "more than 2^31 - 1 blocks";
    const size_t bytes = extent(frames, stride ? stride : frame, frame);
    if (d_in != d_out && overlap(d_out, bytes, d_in, bytes)) return "d_out overlaps d_in without being equal";
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_rs_create(vit_hip_handle h, const vit_hip_rs_params* params, vit_hip_rs_code* out) {
    if (!h || !out) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle or output");
    *out = nullptr;
    if (const char* why = rs_params_invalid(params)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    uint8_t blob[RS_TABLE_BYTES];
    rs_build_tables(params, blob);
    VIT_HIP_ON_DEVICE(h->device);
    vit_hip_rs_code code = nullptr;
    VIT_HIP_NOTHROW((code = new vit_hip_rs_code_s{*params, h->device, nullptr}));
    hipError_t e = hipMalloc((void**)&code->d_tables, RS_TABLE_BYTES);
    if (e == hipSuccess) e = hipMemcpy(code->d_tables, blob, RS_TABLE_BYTES, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (code->d_tables) (void)hipFree(code->d_tables);
        delete code;
        return fail(VIT_HIP_ERR_RUNTIME, std::string("rs table upload: ") + hipGetErrorString(e));
    }
    *out = code;
    return VIT_HIP_OK;
}

void vit_hip_rs_destroy(vit_hip_rs_code code) {
    if (!code) return;
    {
        DeviceGuard guard(code->device);
        (void)hipFree(code->d_tables);
    }
    delete code;
}

int vit_hip_rs_decode_batch(vit_hip_handle h, vit_hip_rs_code code, const uint8_t* d_in, uint8_t* d_out, size_t frame_stride_bytes,
                            size_t rows, size_t max_frames, const uint32_t* d_n_frames, size_t interleave, int32_t* d_status,
                            vit_hip_stream_t stream) {
    if (const char* why = rs_decode_invalid(h, code, d_in, d_out, frame_stride_bytes, rows, max_frames, interleave, d_status))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0) return VIT_HIP_OK;
    const vit_hip_rs_params& p = code->params;
    RsArgs a{};
    a.in = d_in; a.out = d_out; a.n_frames = d_n_frames; a.status = d_status; a.tables = code->d_tables;
    a.n = 255 - p.pad; a.nroots = p.nroots; a.t = p.nroots / 2; a.fcr = p.fcr; a.prim = p.prim;
    a.I = (uint32_t)interleave; a.tiles = (a.I + RS_TILE - 1) / RS_TILE;
    a.stride = frame_stride_bytes ? frame_stride_bytes : (uint64_t)a.n * a.I;
    a.max_frames = max_frames;
    const RsGeometry g = rs_geometry(a.nroots, a.n);
    a.R2 = g.R2; a.G = g.G; a.seg = g.seg; a.base = g.base;
    VIT_HIP_ON_DEVICE(h->device);
    if (rs_launch_decode(a, (uint64_t)rows * max_frames, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "rs decode launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
