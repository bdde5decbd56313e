// scaled_model_tests.cpp -- Decoder::decode_scaled of include/hvc_model.hpp on the GPU path: the planes are what
// hvc_jpeg_decode_scaled gives, and the decoder can be used again afterwards (another scale, then the full decode).
//   scaled_model_tests <golden dir>
#include <fstream>
#include <iostream>
#include <sstream>

#include "hvc_model.hpp"

using namespace hvc_model;

static std::string read_all(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

// the decoder's padded planes against the library call's record
static bool same_as_the_call(Ctx &ctx, const std::string &bits, int scale, const Decoder::t &d) {
    hvc_jpeg_info info;
    std::vector<uint8_t> px((size_t)1 << 20);
    check(hvc_jpeg_decode_scaled(ctx.get(), reinterpret_cast<const uint8_t *>(bits.data()), bits.size(), scale, &info, px.data(), px.size()),
          "hvc_jpeg_decode_scaled");
    const auto planes = d.get_decoded_planes();
    const int n = 8 / scale;
    bool ok = (int)planes.size() == info.n_comp && d.header().info.width == info.width && d.header().info.height == info.height;
    for (int i = 0; ok && i < info.n_comp; i++) {
        const hvc_component &L = info.layout[i];
        ok = planes[i].width() == L.blocks_w * n && planes[i].height() == L.blocks_h * n;
        for (int y = 0; ok && y < planes[i].height(); y++)
            for (int x = 0; ok && x < planes[i].width(); x++) ok = planes[i].data()[(size_t)y * planes[i].width() + x] == px[L.plane_offset + (size_t)y * L.stride + x];
    }
    return ok;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    try {
        Ctx ctx(0);
        const std::string mouse = read_all(std::string(argv[1]) + "/Mouse480.jpg");
        Decoder::t d = Decoder::init(ctx, Decoder::Header::decode(mouse), mouse);
        for (int scale : {2, 8, 4, 4}) { // one scale after another, and one twice: each starts from the file
            d.decode_scaled(scale);
            std::cout << "decode_scaled " << scale << " " << (same_as_the_call(ctx, mouse, scale, d) ? "ok" : "MISMATCH") << "\n";
        }
        d.decode(); // and the full decode after a scaled one
        const auto planes = d.get_decoded_planes();
        const bool ok = planes.size() == 3 && planes[0].width() == 480 && planes[0].height() == 320 && planes[1].width() == 240 &&
                        d.get_yuv_frame().width() == 480 && same_as_the_call(ctx, mouse, 1, d);
        std::cout << "decode after decode_scaled " << (ok ? "ok" : "MISMATCH") << "\n";
        d.decode_scaled(2);
        std::cout << "get_yuv_frame at 1/2 " << (d.get_yuv_frame().width() == 240 && d.get_yuv_frame().height() == 160 ? "ok" : "MISMATCH") << "\n";
    } catch (const Error &e) {
        std::cout << "EXCEPTION " << e.what() << "\n";
        return 1;
    }
    return 0;
}
