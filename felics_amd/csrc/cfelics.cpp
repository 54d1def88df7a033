// cfelics -- compresses an image file to a felics file on the GPU.
// Drop-in for the reference's src/bin/cfelics.rs: same flags, same stdout lines, exit status 1 on
// failure.  The image is decoded on the host, encoded by libfelics on an MI355X, written to disk.
// --index FILE [--segment N] also writes the stream's restart index (felics.h; N pixels per segment, default 65536): stream and
// index then come out of one felics_compress_batch_device_indexed call with n = 1 (8-bit images only: the library refuses others).
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/felics.h"
#include "cli_args.h"
#include "image_io.h"

int main(int argc, char **argv) {
    // libfelics runs its stages on HIP streams of their own: ask the ROCm runtime for enough hardware queues before it
    // starts (an application's choice, not the library's; a value already in the environment wins)
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    CliArgs args = cli_parse(argc, argv, "cfelics", "Compresses an image file to a felics file", "The input file",
                             "The output felics file", CLI_INDEX | CLI_SEGMENT);
    imageio::Image img;
    bool open_failed = false;
    std::string err = imageio::read_image(args.input, img, open_failed);
    if (!err.empty()) {
        printf("%s: %s\n", open_failed ? "Cannot open file" : "Cannot decode image", err.c_str());  // cfelics.rs:39,47
        return 1;
    }
    if (img.channels != 1 && img.channels != 3) {
        printf("Unsupported image format: %s\n", img.color_name().c_str());  // cfelics.rs:70
        return 1;
    }
    printf("Compressing %d-bit %s image...\n", img.bits, img.channels == 1 ? "grayscale" : "rgb");  // cfelics.rs:54-66

    const int color = img.channels == 3 ? FELICS_COLOR_RGB : FELICS_COLOR_GRAY;
    const int depth = img.bits == 16 ? FELICS_DEPTH_16 : FELICS_DEPTH_8;
    felics_ctx *ctx = nullptr;
    int rc = felics_ctx_create(args.device, &ctx);
    if (rc != FELICS_OK) {
        printf("Cannot compress image: %s\n", felics_strerror(rc));
        return 1;
    }
    std::vector<uint8_t> out(img.data.size() + img.data.size() / 2 + 64), index;
    size_t n = 0;
    if (!args.index.empty()) {
        // pixels, stream and index in device memory (the indexed call's interface); a shape that has no index gets a token buffer and
        // the library's refusal
        const size_t cap = felics_max_compressed_size(img.width, img.height, color, depth) + 64;
        const size_t isize = felics_index_size(img.width, img.height, color, depth, (uint32_t)std::min(args.segment, 0xFFFFFFFFul));
        void *d_px = nullptr, *d_out = nullptr, *d_idx = nullptr;
        uint64_t off = 0, len = 0;
        out.resize(cap);
        index.resize(isize);
        const bool up = hipSetDevice(args.device) == hipSuccess && hipMalloc(&d_px, std::max<size_t>(img.data.size(), 16)) == hipSuccess &&
                        hipMalloc(&d_out, cap) == hipSuccess && hipMalloc(&d_idx, std::max<size_t>(isize, 16)) == hipSuccess &&
                        hipMemcpy(d_px, img.data.data(), img.data.size(), hipMemcpyHostToDevice) == hipSuccess;
        rc = up ? felics_compress_batch_device_indexed(ctx, 1, d_px, img.width, img.height, color, depth, d_out, cap,
                                                       (uint32_t)std::min(args.segment, 0xFFFFFFFFul), d_idx, isize, &off, &len)
                : FELICS_E_HIP;
        if (rc == FELICS_OK && (hipMemcpy(out.data(), (const uint8_t *)d_out + off, len, hipMemcpyDeviceToHost) != hipSuccess ||
                                hipMemcpy(index.data(), d_idx, isize, hipMemcpyDeviceToHost) != hipSuccess))
            rc = FELICS_E_HIP;
        n = (size_t)len;
        (void)hipFree(d_px);
        (void)hipFree(d_out);
        (void)hipFree(d_idx);
    } else {
        rc = felics_compress(ctx, img.data.data(), img.width, img.height, color, depth, out.data(), out.size(), &n);
        if (rc == FELICS_E_BUFFER_TOO_SMALL) {
            out.resize(n);
            rc = felics_compress(ctx, img.data.data(), img.width, img.height, color, depth, out.data(), out.size(), &n);
        }
    }
    if (rc != FELICS_OK) {
        const char *detail = felics_last_error(ctx);
        printf("Cannot compress image: %s%s%s\n", felics_strerror(rc), *detail ? ": " : "", detail);  // cfelics.rs:76
        felics_ctx_destroy(ctx);
        return 1;
    }
    felics_ctx_destroy(ctx);
    FILE *f = fopen(args.output.c_str(), "wb");  // File::create, cfelics.rs:28
    if (!f) {
        printf("Cannot compress image: %s\n", strerror(errno));
        return 1;
    }
    const bool ok = fwrite(out.data(), 1, n, f) == n;
    if (fclose(f) != 0 || !ok) {
        printf("Cannot compress image: write failed\n");
        return 1;
    }
    if (!args.index.empty()) {
        f = fopen(args.index.c_str(), "wb");
        if (!f) {
            printf("Cannot write index: %s\n", strerror(errno));
            return 1;
        }
        const bool iok = fwrite(index.data(), 1, index.size(), f) == index.size();
        if (fclose(f) != 0 || !iok) {
            printf("Cannot write index: write failed\n");
            return 1;
        }
    }
    return 0;
}
