// `raytrace` -- the replacement for the reference's main.rs:13-60.
//
// Reads a scene file in the reference grammar (default test_scene.txt, as
// main.rs:16), renders it on one or more GPUs through the C ABI, and writes the
// reference's BMP (default out.bmp, main.rs:34).  Multi-GPU: image rows are
// dealt in interleaved bands, one host thread + one rt_ctx per device, each
// device renders its bands into its own buffer and the host gathers them into
// the frame (no collective: pixels are independent, main.rs:45-57).
//
//   raytrace [--scene FILE] [--out FILE] [--width W] [--height H] [--spp N]
//            [--max-depth D] [--gpus N] [--band ROWS] [--jitter random|center] [--seed N]
//            [--algo auto|wavefront|wavefront-aa|path|lds|global]
//            [--progressive K] [--checkpoint FILE] [--aov PREFIX]
//            [--until-noise T] [--noise-floor F] [--noise-pixels P] [--variance FILE.pfm]
//            [--denoise ITER] [--denoise-flags normal,depth,color,demodulate|none]
//            [--denoise-variance SIGMA] [--denoise-variance-floor F]
//
// --denoise ITER: the image goes through the edge-avoiding a-trous filter (rt_denoise, ITER passes 1..8) before it is
// written: the frame is rendered with its f32 colours, the first-hit feature buffers with the same --spp, --jitter
// and --seed (rt_render_aov), and the BMP holds the filter's bytes.  --denoise-flags (default normal,depth) names the
// guides; normal_squarings 5, sigma_depth 0.05, sigma_color 1.0.  With --progressive every written frame is
// denoised.  Single-device; a DepthOfFieldCamera has no feature buffers and is refused.
// --denoise ITER --denoise-variance SIGMA [--denoise-variance-floor F]: the variance-guided filter (rt_denoise_var,
// sigma_variance SIGMA, variance_floor F, default 2^-20).  The frame is rendered through an accumulator that keeps the
// sums of squares (without --progressive: one rt_render_accumulate call, whose image is the one-shot render's bit
// for bit), rt_accum_noise gives the variance of every pixel's mean (--noise-floor applies), and that guides the
// filter beside the feature buffers.  With --progressive every written frame of at least 2 samples goes through it; a
// frame of 1 sample has no variance, goes through the plain filter and says so on stderr.  Needs --jitter random
// and --spp of at least 2.  --until-noise, --variance and --checkpoint combine with it: they read the same
// accumulator (the stop rule is asked on the unfiltered samples; --variance writes the image the filter was guided by),
// and a --noise-floor that is not finite and > 0 is refused as it is for them.
// --aov PREFIX: instead of the image, the first-hit feature buffers of the frame (rt_render_aov; --spp, --jitter,
// --seed, --width, --height apply) as PFM files (portable float map: "PF" 3 channels / "Pf" 1 channel, width
// height, scale -1.0 = little-endian, rows bottom-up, which is the library's row order): PREFIX.depth.pfm,
// PREFIX.normal.pfm, PREFIX.albedo.pfm, PREFIX.coverage.pfm and PREFIX.object.pfm (the id as a float; ids are
// below 2^24).  Single-device.
// --progressive K: the frame's samples in steps of K (rt_render_accumulate; main.rs:47-56 split over
// calls); after every step --out is rewritten (a temporary name, renamed) with the image of the samples
// so far and "samples done/total" goes to stderr.  --checkpoint FILE: FILE is written after every step
// (the running sums, rt_checkpoint_write); a run that finds FILE continues from it when its options and
// the scene's hash (FNV-1a 64 of the scene text) match, and refuses otherwise.  Both are single-device.
// --progressive K --until-noise T [--noise-floor F] [--noise-pixels P]: the accumulator also keeps the sums of
// squares (rt_accum_create_moments); after every step from 2 samples on, rt_accum_noise counts the pixels whose
// relative error sqrt(variance of the mean) / (F + |mean|) is not <= T (F default 0.001), "noise above N" goes
// to stderr, and the run stops when N <= P (default 0) or at --spp (a resumed run asks before its first step, and
// then only writes the image of the samples it holds); the last line names the final sample count.
// --variance FILE.pfm writes the variance image of the final samples (3 channels, rows as --aov's files).  With
// either, --checkpoint writes format version 2 (sums and squares) and resumes only from a file of that kind, as a
// run without them resumes only from version 1; a file of the other kind is left alone until the first step
// overwrites it, and the run starts fresh with a message.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "raytrace_amd.h"

namespace {

struct Args {
    std::string scene = "test_scene.txt", out = "out.bmp";
    long width = -1, height = -1, spp = -1;
    unsigned max_depth = 4;        // raytrace.rs:18
    int gpus = 1;
    unsigned band = 16;
    int algo = RT_ALGO_AUTO;
    int jitter = RT_JITTER_RANDOM;     // main.rs:51-52 jitters every sample; --jitter center = parity mode
    unsigned long long seed = 1;       // keyed draws (the reference seeds from OS entropy, main.rs:43)
    long progressive = 0;              // samples per step (0: one render)
    std::string checkpoint;
    double until_noise = 0;            // --until-noise T (0: run to --spp)
    double noise_floor = 1e-3;
    long noise_pixels = 0;
    std::string variance;              // --variance FILE.pfm
    bool moments() const { return until_noise != 0 || !variance.empty() || denoise_var; }
    std::string aov;                   // --aov PREFIX: write the feature buffers instead of the image
    long denoise = 0;                  // --denoise ITER: filter passes (0: off)
    unsigned denoise_flags = RT_DN_NORMAL | RT_DN_DEPTH;
    bool bad_denoise_flags = false;
    bool denoise_var = false;          // --denoise-variance SIGMA: the variance-guided filter
    double sigma_variance = 0, variance_floor = 1.0 / 1048576.0;
};

// "normal,depth,color,demodulate" (any subset, any order) or "none" -> rt_denoise_flags; false: an unknown word.
bool parse_denoise_flags(const std::string& text, unsigned& flags) {
    flags = 0;
    if (text == "none") return true;
    std::stringstream ss(text);
    std::string w;
    while (std::getline(ss, w, ',')) {
        if (w == "normal") flags |= RT_DN_NORMAL;
        else if (w == "depth") flags |= RT_DN_DEPTH;
        else if (w == "color") flags |= RT_DN_COLOR;
        else if (w == "demodulate") flags |= RT_DN_DEMODULATE;
        else return false;
    }
    return true;
}

bool parse_args(int argc, char** argv, Args& a) {
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i];
        auto val = [&]() -> const char* { return i + 1 < argc ? argv[++i] : nullptr; };
        const char* v = nullptr;
        if (k == "--scene" && (v = val())) a.scene = v;
        else if (k == "--out" && (v = val())) a.out = v;
        else if (k == "--width" && (v = val())) a.width = std::atol(v);
        else if (k == "--height" && (v = val())) a.height = std::atol(v);
        else if (k == "--spp" && (v = val())) a.spp = std::atol(v);
        else if (k == "--max-depth" && (v = val())) a.max_depth = static_cast<unsigned>(std::atol(v));
        else if (k == "--gpus" && (v = val())) a.gpus = std::atoi(v);
        else if (k == "--band" && (v = val())) a.band = static_cast<unsigned>(std::atol(v));
        else if (k == "--seed" && (v = val())) a.seed = std::strtoull(v, nullptr, 0);
        else if (k == "--progressive" && (v = val())) a.progressive = std::atol(v);
        else if (k == "--checkpoint" && (v = val())) a.checkpoint = v;
        else if (k == "--until-noise" && (v = val())) a.until_noise = std::atof(v);
        else if (k == "--noise-floor" && (v = val())) a.noise_floor = std::atof(v);
        else if (k == "--noise-pixels" && (v = val())) a.noise_pixels = std::atol(v);
        else if (k == "--variance" && (v = val())) a.variance = v;
        else if (k == "--aov" && (v = val())) a.aov = v;
        else if (k == "--denoise" && (v = val())) a.denoise = std::atol(v);
        else if (k == "--denoise-flags" && (v = val())) a.bad_denoise_flags = !parse_denoise_flags(v, a.denoise_flags);
        else if (k == "--denoise-variance" && (v = val())) { a.denoise_var = true; a.sigma_variance = std::atof(v); }
        else if (k == "--denoise-variance-floor" && (v = val())) a.variance_floor = std::atof(v);
        else if (k == "--jitter" && (v = val())) a.jitter = std::string(v) == "center" ? RT_JITTER_CENTER : RT_JITTER_RANDOM;
        else if (k == "--algo" && (v = val())) {
            std::string s = v;
            a.algo = s == "lds" ? RT_ALGO_BRUTE_LDS : s == "global" ? RT_ALGO_BRUTE_GLOBAL
                   : s == "wavefront" ? RT_ALGO_WAVEFRONT : s == "wavefront-aa" ? RT_ALGO_WAVEFRONT_AA
                   : s == "path" ? RT_ALGO_PATH : RT_ALGO_AUTO;
        } else {
            std::fprintf(stderr, "usage: raytrace [--scene FILE] [--out FILE] [--width W] [--height H] [--spp N]\n"
                                 "                [--max-depth D] [--gpus N] [--band ROWS] [--jitter random|center]\n"
                                 "                [--seed N] [--algo auto|wavefront|wavefront-aa|path|lds|global]\n"
                                 "                [--progressive K] [--checkpoint FILE] [--aov PREFIX]\n"
                                 "                [--until-noise T] [--noise-floor F] [--noise-pixels P] [--variance FILE.pfm]\n"
                                 "                [--denoise ITER] [--denoise-flags normal,depth,color,demodulate|none]\n"
                                 "                [--denoise-variance SIGMA] [--denoise-variance-floor F]\n");
            return false;
        }
    }
    return true;
}

uint64_t fnv1a64(const std::string& text) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char ch : text) h = (h ^ ch) * 0x100000001b3ull;
    return h;
}

// --denoise: the guides of the frame (rendered once, with the image's spp, jitter and seed) and the filter's settings.
struct Denoiser {
    std::vector<float> normal, depth, albedo;
    rt_denoise_params p{};
    // the guides from rt_render_aov; false: refused (rt_last_error(ctx) says why, e.g. a DepthOfFieldCamera)
    bool setup(rt_ctx* ctx, const Args& a, uint32_t W, uint32_t H, uint32_t spp, uint32_t pitch) {
        const size_t n = static_cast<size_t>(W) * H;
        normal.resize(3 * n); depth.resize(n); albedo.resize(3 * n);
        p.width = W; p.height = H; p.iterations = static_cast<uint32_t>(a.denoise); p.flags = a.denoise_flags;
        p.normal_squarings = 5; p.variant = 0; p.bgr_pitch = pitch;
        p.sigma_color = 1.0; p.sigma_depth = 0.05;
        rt_render_opts o;
        rt_render_opts_default(&o, W, H);
        o.spp = spp; o.jitter = a.jitter; o.seed = a.seed;
        const rt_aov_buffers b{depth.data(), normal.data(), albedo.data(), nullptr, nullptr};
        return rt_render_aov(ctx, &o, RT_AOV_DEPTH | RT_AOV_NORMAL | RT_AOV_ALBEDO, &b, nullptr) == RT_OK;
    }
    // rgb (tight f32) -> the BMP rows of `frame`
    bool run(rt_ctx* ctx, const float* rgb, uint8_t* frame) const {
        const rt_denoise_inputs in{rgb, normal.data(), depth.data(), albedo.data()};
        return rt_denoise(ctx, &p, &in, nullptr, frame) == RT_OK;
    }
    // --denoise-variance: the same with the variance of the mean (tight f32, 3 channels) as one more guide
    bool run_var(rt_ctx* ctx, const Args& a, const float* rgb, const float* variance, uint8_t* frame) const {
        const rt_denoise_inputs in{rgb, normal.data(), depth.data(), albedo.data()};
        const rt_denoise_variance var{variance, nullptr, a.sigma_variance, a.variance_floor};
        return rt_denoise_var(ctx, &p, &in, &var, nullptr, frame) == RT_OK;
    }
};

// --denoise without --progressive: one device, the whole frame: colours, guides, filter, BMP.
int run_denoised(const Args& a, rt_scene* scene, uint32_t W, uint32_t H, uint32_t spp) {
    uint32_t pitch = 0;
    uint8_t hdr[122];
    rt_bmp_header(hdr, W, H, &pitch);
    rt_ctx* ctx = nullptr;
    if (rt_ctx_create(0, &ctx) != RT_OK) { std::printf("error: %s\n", rt_last_error(nullptr)); return 1; }
    auto done_with = [&](int code) {
        rt_ctx_destroy(ctx);
        return code;
    };
    if (rt_scene_upload(ctx, scene) != RT_OK) { std::printf("error: %s\n", rt_last_error(ctx)); return done_with(1); }
    Denoiser dn;
    if (!dn.setup(ctx, a, W, H, spp, pitch)) { std::printf("error: --denoise: %s\n", rt_last_error(ctx)); return done_with(2); }
    rt_render_opts o;
    rt_render_opts_default(&o, W, H);
    o.max_depth = a.max_depth; o.spp = spp; o.algo = a.algo; o.jitter = a.jitter; o.seed = a.seed;
    o.flags = RT_OUT_RGB_F32;
    std::vector<float> rgb(static_cast<size_t>(W) * H * 3);
    std::vector<uint8_t> frame(static_cast<size_t>(pitch) * H, 0);
    rt_stats st{};
    if (rt_render(ctx, &o, rgb.data(), nullptr, &st) != RT_OK) { std::printf("error: %s\n", rt_last_error(ctx)); return done_with(1); }
    if (!dn.run(ctx, rgb.data(), frame.data())) { std::printf("error: --denoise: %s\n", rt_last_error(ctx)); return done_with(1); }
    if (rt_write_bmp(a.out.c_str(), W, H, frame.data(), pitch) != RT_OK) {
        std::printf("error: %s\n", rt_last_error(nullptr));
        return done_with(1);
    }
    std::fprintf(stderr, "%ux%u spp=%u depth=%u gpus=1 denoise %ld (flags 0x%x): %llu rays, kernel %.3f ms\n", W, H, spp, a.max_depth,
                 a.denoise, a.denoise_flags, static_cast<unsigned long long>(st.rays), st.kernel_ms);
    return done_with(0);
}

bool write_pfm(const std::string& path, uint32_t W, uint32_t H, int channels, const float* data);

// --progressive / --checkpoint / --until-noise / --variance / --denoise-variance: one device, the whole frame in one
// accumulator, `total` samples in steps (without --progressive: one step).
int run_progressive(const Args& a, rt_scene* scene, const std::string& text, uint32_t W, uint32_t H, uint32_t total) {
    uint32_t pitch = 0;
    uint8_t hdr[122];
    rt_bmp_header(hdr, W, H, &pitch);
    rt_ctx* ctx = nullptr;
    rt_accum* acc = nullptr;
    auto done_with = [&](int code) {
        rt_accum_destroy(acc);
        rt_ctx_destroy(ctx);
        return code;
    };
    if (rt_ctx_create(0, &ctx) != RT_OK) { std::printf("error: %s\n", rt_last_error(nullptr)); return 1; }
    if (rt_scene_upload(ctx, scene) != RT_OK) { std::printf("error: %s\n", rt_last_error(ctx)); return done_with(1); }
    rt_render_opts o;
    rt_render_opts_default(&o, W, H);
    o.max_depth = a.max_depth; o.jitter = a.jitter; o.seed = a.seed;
    const bool moments = a.moments();
    if ((moments ? rt_accum_create_moments(ctx, &o, &acc) : rt_accum_create(ctx, &o, &acc)) != RT_OK) {
        std::printf("error: %s\n", rt_last_error(ctx));
        return done_with(1);
    }
    const uint64_t hash = fnv1a64(text);
    const size_t n_doubles = static_cast<size_t>(W) * H * 3;
    std::vector<double> sums, squares;
    uint32_t done = 0;
    if (!a.checkpoint.empty()) {
        sums.resize(n_doubles);
        if (moments) squares.resize(n_doubles);
        rt_render_opts co;
        uint64_t ch = 0;
        uint32_t cs = 0;
        // the file of this run's kind: version 2 (sums and squares) with moments, version 1 without
        auto read_ckpt = [&](bool m, double* s, double* q, size_t cap) {
            return m ? rt_checkpoint_read_moments(a.checkpoint.c_str(), &co, &ch, &cs, s, q, cap)
                     : rt_checkpoint_read(a.checkpoint.c_str(), &co, &ch, &cs, s, cap);
        };
        int rc = read_ckpt(moments, nullptr, nullptr, 0);
        if (rc == RT_E_INVALID && read_ckpt(!moments, nullptr, nullptr, 0) == RT_OK) {
            std::fprintf(stderr, "checkpoint %s holds %s: not resumed, starting fresh\n", a.checkpoint.c_str(),
                         moments ? "sums without squares (format version 1)" : "sums and squares (format version 2)");
            rc = RT_E_IO;
        }
        if (rc == RT_OK) {
            const uint32_t cband = co.band ? co.band : 1, cstride = co.band_stride ? co.band_stride : 1;
            const bool same = co.width == W && co.height == H && co.x0 == 0 && co.tile_w == W && co.y0 == 0 && co.tile_h == H &&
                              cband == 1 && cstride == 1 && co.band_phase == 0 && co.max_depth == o.max_depth &&
                              co.jitter == o.jitter && co.seed == o.seed;
            if (!same || ch != hash || cs > total) {
                std::printf("error: checkpoint %s was written for %s: not resumed (remove it to start again)\n", a.checkpoint.c_str(),
                            !same ? "other options" : ch != hash ? "another scene" : "fewer samples than it holds");
                return done_with(1);
            }
            if (read_ckpt(moments, sums.data(), moments ? squares.data() : nullptr, sums.size()) != RT_OK ||
                (moments ? rt_accum_upload_moments(ctx, acc, sums.data(), squares.data(), sums.size(), cs)
                         : rt_accum_upload(ctx, acc, sums.data(), sums.size(), cs)) != RT_OK) {
                std::printf("error: checkpoint %s: %s\n", a.checkpoint.c_str(), rt_last_error(nullptr));
                return done_with(1);
            }
            done = cs;
            std::fprintf(stderr, "resuming %s at %u samples\n", a.checkpoint.c_str(), done);
        } else if (rc != RT_E_IO) {
            std::printf("error: checkpoint %s: %s\n", a.checkpoint.c_str(), rt_last_error(nullptr));
            return done_with(1);
        }
    }
    Denoiser dn;                       // --denoise: the guides once, at the frame's sample count
    std::vector<float> rgb, dn_var;
    if (a.denoise > 0) {
        if (!dn.setup(ctx, a, W, H, total, pitch)) { std::printf("error: --denoise: %s\n", rt_last_error(ctx)); return done_with(2); }
        rgb.resize(n_doubles);
        if (a.denoise_var) dn_var.resize(n_doubles);
    }
    const uint32_t step = a.progressive > 0 ? static_cast<uint32_t>(std::min<long>(a.progressive, total)) : total;
    std::vector<uint8_t> frame(static_cast<size_t>(pitch) * H, 0);
    // --denoise: the image of the `have` samples so far through the filter; variance-guided from 2 samples on
    auto denoised = [&](uint32_t have) {
        if (rt_accum_resolve_host(ctx, acc, pitch, rgb.data(), nullptr) != RT_OK) return false;
        if (!a.denoise_var) return dn.run(ctx, rgb.data(), frame.data());
        if (have < 2) {
            std::fprintf(stderr, "samples %u: no variance yet, the plain filter\n", have);
            return dn.run(ctx, rgb.data(), frame.data());
        }
        uint64_t above = 0;
        return rt_accum_noise_host(ctx, acc, a.noise_floor, 1.0, dn_var.data(), nullptr, &above) == RT_OK &&
               dn.run_var(ctx, a, rgb.data(), dn_var.data(), frame.data());
    };
    const std::string tmp = a.out + ".tmp";
    uint64_t rays = 0;
    double kms = 0;
    auto t0 = std::chrono::steady_clock::now();
    // the stop rule: few enough pixels still above the threshold; 1 converged, 0 not, -1 an error
    auto converged = [&]() {
        uint64_t above = 0;
        if (rt_accum_noise_host(ctx, acc, a.noise_floor, a.until_noise, nullptr, nullptr, &above) != RT_OK) return -1;
        std::fprintf(stderr, "noise above %llu\n", static_cast<unsigned long long>(above));
        return above <= static_cast<uint64_t>(std::max(0l, a.noise_pixels)) ? 1 : 0;
    };
    // a resumed render may have converged already: the rule is asked before any more samples are traced
    bool stop = false;
    if (a.until_noise != 0 && done >= 2 && done < total) {
        const int cv = converged();
        if (cv < 0) { std::printf("error: %s\n", rt_last_error(ctx)); return done_with(1); }
        stop = cv == 1;
    }
    for (bool first = true; first || (done < total && !stop); first = false) {
        const uint32_t n = stop ? 0u : std::min(step, total - done);
        rt_stats st{};
        if (n && (rt_render_accumulate(ctx, acc, n, a.algo, 0, nullptr) != RT_OK || rt_ctx_stats(ctx, &st) != RT_OK)) {
            std::printf("error: %s\n", rt_last_error(ctx));
            return done_with(1);
        }
        done += n;
        rays += st.rays;
        kms += st.kernel_ms;
        if (done == 0) break;
        // the image of the samples so far, under a temporary name first: --out is always a whole image
        if (a.denoise > 0 ? !denoised(done) : rt_accum_resolve_host(ctx, acc, pitch, nullptr, frame.data()) != RT_OK) {
            std::printf("error: %s\n", rt_last_error(ctx));
            return done_with(1);
        }
        if (rt_write_bmp(tmp.c_str(), W, H, frame.data(), pitch) != RT_OK || std::rename(tmp.c_str(), a.out.c_str()) != 0) {
            std::printf("error: cannot write %s\n", a.out.c_str());
            return done_with(1);
        }
        if (!a.checkpoint.empty() && n) {
            uint32_t cs = 0;
            if (rt_accum_download(ctx, acc, sums.data(), sums.size(), &cs) != RT_OK ||
                (moments && rt_accum_download_moments(ctx, acc, squares.data(), squares.size()) != RT_OK) ||
                (moments ? rt_checkpoint_write_moments(a.checkpoint.c_str(), &o, hash, cs, sums.data(), squares.data(), sums.size())
                         : rt_checkpoint_write(a.checkpoint.c_str(), &o, hash, cs, sums.data(), sums.size())) != RT_OK) {
                std::printf("error: checkpoint %s: %s\n", a.checkpoint.c_str(), rt_last_error(nullptr));
                return done_with(1);
            }
        }
        std::fprintf(stderr, "samples %u/%u\n", done, total);
        if (a.until_noise != 0 && done >= 2 && n) {
            const int cv = converged();
            if (cv < 0) { std::printf("error: %s\n", rt_last_error(ctx)); return done_with(1); }
            if (cv == 1) break;
        }
    }
    if (a.until_noise != 0) std::fprintf(stderr, "stopped at %u samples\n", done);
    if (!a.variance.empty()) {
        std::vector<float> var(n_doubles);
        uint64_t above = 0;
        if (rt_accum_noise_host(ctx, acc, a.noise_floor, a.until_noise != 0 ? a.until_noise : 1.0, var.data(), nullptr, &above) != RT_OK) {
            std::printf("error: --variance: %s\n", rt_last_error(ctx));
            return done_with(1);
        }
        if (!write_pfm(a.variance, W, H, 3, var.data())) { std::printf("error: cannot write %s\n", a.variance.c_str()); return done_with(1); }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "%ux%u spp=%u depth=%u gpus=1 progressive: %llu rays, kernels %.3f ms, wall %.3f s\n", W, H, done,
                 a.max_depth, static_cast<unsigned long long>(rays), kms, sec);
    return done_with(0);
}

// One PFM file: `channels` (1 or 3) floats per pixel, rows in the library's order (row 0 = the image bottom).
bool write_pfm(const std::string& path, uint32_t W, uint32_t H, int channels, const float* data) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t n = static_cast<size_t>(W) * H * channels;
    bool ok = std::fprintf(f, "%s\n%u %u\n-1.0\n", channels == 3 ? "PF" : "Pf", W, H) > 0;
    ok = ok && std::fwrite(data, sizeof(float), n, f) == n;
    return (std::fclose(f) == 0) && ok;
}

// --aov PREFIX: one device, the whole frame, every channel.
int run_aov(const Args& a, rt_scene* scene, uint32_t W, uint32_t H, uint32_t spp) {
    rt_ctx* ctx = nullptr;
    if (rt_ctx_create(0, &ctx) != RT_OK) { std::printf("error: %s\n", rt_last_error(nullptr)); return 1; }
    auto done_with = [&](int code) {
        rt_ctx_destroy(ctx);
        return code;
    };
    if (rt_scene_upload(ctx, scene) != RT_OK) { std::printf("error: %s\n", rt_last_error(ctx)); return done_with(1); }
    rt_render_opts o;
    rt_render_opts_default(&o, W, H);
    o.spp = spp; o.jitter = a.jitter; o.seed = a.seed;
    const size_t n = static_cast<size_t>(W) * H;
    std::vector<float> depth(n), normal(3 * n), albedo(3 * n), coverage(n), idf(n);
    std::vector<int32_t> object(n);
    const rt_aov_buffers b{depth.data(), normal.data(), albedo.data(), coverage.data(), object.data()};
    rt_stats st{};
    const uint32_t all = RT_AOV_DEPTH | RT_AOV_NORMAL | RT_AOV_ALBEDO | RT_AOV_COVERAGE | RT_AOV_OBJECT;
    if (rt_render_aov(ctx, &o, all, &b, &st) != RT_OK) { std::printf("error: %s\n", rt_last_error(ctx)); return done_with(1); }
    for (size_t i = 0; i < n; ++i) idf[i] = static_cast<float>(object[i]);
    const struct { const char* name; int channels; const float* data; } files[] = {
        {"depth", 1, depth.data()}, {"normal", 3, normal.data()}, {"albedo", 3, albedo.data()},
        {"coverage", 1, coverage.data()}, {"object", 1, idf.data()}};
    for (const auto& f : files) {
        const std::string path = a.aov + "." + f.name + ".pfm";
        if (!write_pfm(path, W, H, f.channels, f.data)) { std::printf("error: cannot write %s\n", path.c_str()); return done_with(1); }
    }
    std::fprintf(stderr, "%ux%u spp=%u aov: %llu rays, kernel %.3f ms\n", W, H, spp, static_cast<unsigned long long>(st.rays),
                 st.kernel_ms);
    return done_with(0);
}

}  // namespace

int main(int argc, char** argv) {
    Args a;
    if (!parse_args(argc, argv, a)) return 2;
    std::ifstream f(a.scene, std::ios::binary);
    if (!f) { std::printf("error: cannot open %s\n", a.scene.c_str()); return 1; }   // main.rs:18
    std::stringstream ss;
    ss << f.rdbuf();
    std::string text = ss.str();
    rt_scene* scene = nullptr;
    char err[512];
    if (rt_scene_parse(text.data(), text.size(), &scene, err, sizeof err) != RT_OK) {
        std::printf("error: %s\n", err);                                              // main.rs:28
        return 1;
    }
    rt_scene_desc d;
    rt_scene_get_desc(scene, &d);
    const uint32_t W = a.width > 0 ? static_cast<uint32_t>(a.width) : d.width;
    const uint32_t H = a.height > 0 ? static_cast<uint32_t>(a.height) : d.height;
    const uint32_t spp = a.spp > 0 ? static_cast<uint32_t>(a.spp) : d.antialias;
    int ndev = 0;
    rt_device_count(&ndev);
    if (ndev < 1) { std::printf("error: no GPU\n"); return 1; }
    if (a.denoise_var) {
        if (a.denoise == 0) { std::printf("error: --denoise-variance guides the filter of --denoise ITER: name the passes\n"); return 2; }
        if (!(a.sigma_variance > 0) || !std::isfinite(a.sigma_variance) || !(a.variance_floor > 0) || !std::isfinite(a.variance_floor)) {
            std::printf("error: --denoise-variance and --denoise-variance-floor take finite values > 0\n");
            return 2;
        }
        if (a.jitter != RT_JITTER_RANDOM) {
            std::printf("error: --denoise-variance needs --jitter random (samples through one point have no variance)\n");
            return 2;
        }
        if (spp < 2) { std::printf("error: --denoise-variance needs --spp of at least 2 (a variance of 2 samples)\n"); return 2; }
    }
    if (a.denoise != 0 || a.bad_denoise_flags) {
        if (a.bad_denoise_flags) {
            std::printf("error: --denoise-flags takes normal, depth, color, demodulate (comma-separated) or none\n");
            return 2;
        }
        if (a.denoise < 1 || a.denoise > 8) { std::printf("error: --denoise takes 1..8 passes\n"); return 2; }
        if (a.gpus > 1) {
            std::printf("error: --denoise filters on one device: not with --gpus %d\n", a.gpus);
            return 2;
        }
        if (!a.aov.empty()) { std::printf("error: --denoise filters the image: not with --aov\n"); return 2; }
        if (spp == 0) { std::printf("error: --spp is 0 and the scene's antialias is 0\n"); return 1; }
        if (a.progressive <= 0 && a.checkpoint.empty() && !a.moments()) {
            const int rc = run_denoised(a, scene, W, H, spp);
            rt_scene_free(scene);
            return rc;
        }
    }
    if (!a.aov.empty()) {
        if (a.gpus > 1) {
            std::printf("error: --aov renders on one device: not with --gpus %d\n", a.gpus);
            return 2;
        }
        if (a.progressive > 0 || !a.checkpoint.empty() || a.moments()) {
            std::printf("error: --aov writes the feature buffers of one render: not with --progressive, --checkpoint, "
                        "--until-noise or --variance\n");
            return 2;
        }
        if (spp == 0) { std::printf("error: --spp is 0 and the scene's antialias is 0\n"); return 1; }
        const int rc = run_aov(a, scene, W, H, spp);
        rt_scene_free(scene);
        return rc;
    }
    if (a.moments()) {
        if (a.until_noise != 0 && (!(a.until_noise > 0) || !std::isfinite(a.until_noise) || a.progressive <= 0)) {
            std::printf("error: --until-noise takes a finite threshold > 0 and needs --progressive K (the stop rule is asked after every step)\n");
            return 2;
        }
        if (!(a.noise_floor > 0) || !std::isfinite(a.noise_floor) || a.noise_pixels < 0) {
            std::printf("error: --noise-floor takes a finite value > 0, --noise-pixels a count >= 0\n");
            return 2;
        }
    }
    if (a.progressive > 0 || !a.checkpoint.empty() || a.moments()) {
        if (a.gpus > 1) {
            std::printf("error: --progressive, --checkpoint, --until-noise and --variance render on one device: not with --gpus %d\n", a.gpus);
            return 2;
        }
        if (a.moments() && spp < 2) { std::printf("error: --until-noise and --variance need --spp of at least 2 (a variance of 2 samples)\n"); return 2; }
        if (spp == 0) { std::printf("error: --spp is 0 and the scene's antialias is 0\n"); return 1; }
        const int rc = run_progressive(a, scene, text, W, H, spp);
        rt_scene_free(scene);
        return rc;
    }
    const int G = std::max(1, std::min(a.gpus, ndev));
    const uint32_t band = std::max(1u, a.band);
    uint32_t pitch = 0;
    uint8_t hdr[122];
    rt_bmp_header(hdr, W, H, &pitch);
    std::vector<uint8_t> frame(static_cast<size_t>(pitch) * H, 0);
    std::vector<int> rc(G, RT_OK);
    std::vector<rt_stats> st(G);
    std::vector<std::string> errs(G);
    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g) {
        th.emplace_back([&, g]() {
            rt_ctx* ctx = nullptr;
            if ((rc[g] = rt_ctx_create(g, &ctx)) != RT_OK) { errs[g] = rt_last_error(nullptr); return; }
            if ((rc[g] = rt_scene_upload(ctx, scene)) != RT_OK) { errs[g] = rt_last_error(ctx); rt_ctx_destroy(ctx); return; }
            // rows of this device: bands g, g+G, g+2G, ...
            // full bands only go through the banded mapping; a ragged last band is rendered separately
            const uint32_t full_bands = H / band;
            uint32_t my_full = 0;
            for (uint32_t b = g; b < full_bands; b += G) ++my_full;
            // every device writes its bands straight into their rows of the shared frame (RT_OUT_FRAME_ROWS:
            // the library's copies of one band overlap the render of the others); the bands are disjoint rows
            rt_render_opts o;
            rt_render_opts_default(&o, W, H);
            o.max_depth = a.max_depth; o.spp = spp; o.algo = a.algo; o.jitter = a.jitter; o.seed = a.seed;
            o.flags = RT_OUT_BGR_U8 | RT_OUT_FRAME_ROWS; o.bgr_pitch = pitch;
            o.band = band; o.band_stride = G; o.band_phase = g; o.tile_h = my_full * band;
            if (o.tile_h && ((rc[g] = rt_ctx_reserve(ctx, &o, 1, nullptr)) != RT_OK ||
                             (rc[g] = rt_render(ctx, &o, nullptr, frame.data(), &st[g])) != RT_OK)) {
                errs[g] = rt_last_error(ctx); rt_ctx_destroy(ctx); return;
            }
            if (H % band && full_bands % G == static_cast<uint32_t>(g)) {   // the ragged last band
                rt_render_opts t;
                rt_render_opts_default(&t, W, H);
                t.max_depth = a.max_depth; t.spp = spp; t.algo = a.algo; t.jitter = a.jitter; t.seed = a.seed;
                t.flags = RT_OUT_BGR_U8 | RT_OUT_FRAME_ROWS; t.bgr_pitch = pitch;
                t.y0 = full_bands * band; t.tile_h = H % band;
                rt_stats ts{};
                if ((rc[g] = rt_render(ctx, &t, nullptr, frame.data(), &ts)) != RT_OK) {
                    errs[g] = rt_last_error(ctx); rt_ctx_destroy(ctx); return;
                }
                st[g].rays += ts.rays; st[g].shadow_rays += ts.shadow_rays; st[g].kernel_ms += ts.kernel_ms;
            }
            rt_ctx_destroy(ctx);
        });
    }
    for (auto& t : th) t.join();
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t rays = 0;
    double kms = 0;
    for (int g = 0; g < G; ++g) {
        if (rc[g] != RT_OK) { std::printf("error: gpu %d: %s\n", g, errs[g].c_str()); return 1; }
        rays += st[g].rays;
        kms = std::max(kms, st[g].kernel_ms);
    }
    if (rt_write_bmp(a.out.c_str(), W, H, frame.data(), pitch) != RT_OK) {
        std::printf("error: %s\n", rt_last_error(nullptr));
        return 1;
    }
    std::fprintf(stderr, "%ux%u spp=%u depth=%u gpus=%d: %llu rays, max kernel %.3f ms (%.1f Mrays/s), wall %.3f s\n",
                 W, H, spp, a.max_depth, G, static_cast<unsigned long long>(rays), kms,
                 kms > 0 ? rays / (kms * 1e3) : 0.0, sec);
    rt_scene_free(scene);
    return 0;
}
