// gpu.cpp -- ./gpu <img-path> <psf-length> <psf-angle> | auto auto [--any-blur] | defocus <radius|auto> | blind <size>  [--out file] [--mode fast|parity] [--norm padded|cropped] [--host-epilogue]
//           [--cls gamma|auto] [--k K|auto] [--reg gcv|discrepancy] [--sigma s] [--pad zero|smooth] [--rl iterations|auto [--accel] [--rl-tv lambda [--rl-tv-eps e] [--rl-tv-color]] [--free-boundary [--mask mask.png] [--frame img2 L2 A2 ... [--register [--max-shift s]]]] [--rl-max n] [--rl-stop residual|kl] [--gain g] [--rl-check c]] [--tv mu [--tv-iters n] [--tv-rho r] [--tv-color | --free-boundary [--mask mask.png]]]
// `--rl n|--tv mu --free-boundary --tile T [--overlap O]`: the leg is fft_gpu::restoreTiled_RGB -- overlapping T x T tiles (O pixels shared, default T / 8),
// each restored as a crop of a larger scene with the PSF centred, blended and normalised over the picture; one PSF, --mask as before.
// `--tv mu --free-boundary`: the TV leg is fft_gpu::tvDeblurFree_RGB (the picture is a crop of a larger scene; --mask as for --rl); --tv-color has no such form.
// `--tv auto [--sigma s] [--tv-tau t] [--tv-iters n] [--tv-rho r] [--mask mask.png]`: the TV leg is fft_gpu::tvDeblurAuto_RGB -- the free-boundary
// iteration with mu chosen in every step from the noise level (--sigma, else estimated per channel; the ball is t sigma^2 S, t default 1; n default
// 100), printed per channel as `total-variation: sigma S target T mu M discrepancy D`.  It works with `auto auto`; --tv-color, --rl, --cls and
// --mode parity beside it are refused.
// `--tv mu --poisson [--background b] [--tv-iters n] [--tv-rho r] [--mask mask.png] [--tv-color]`: the TV leg is fft_gpu::tvDeblurPoisson_RGB -- the
// free-boundary iteration with the Poisson likelihood as its data term (photon-limited pictures; b is the known level under the counts, default
// 0; mu = photons per unit times the weight wanted).  --poisson implies --free-boundary; --tv-color couples the channels.  It works with `auto
// auto`; --tv auto, --rl, --cls, --tile and --mode parity beside it are refused with the usage text, before the picture is read.
// `auto auto` for length and angle: the blur is estimated first (fft_gpu::estimateMotionBlur on the per-pixel mean of B, G and R),
// printed as `estimate: length L angle A confidence C`, and the run then goes on exactly as `./gpu <img-path> L A` would.
// `--cls auto` (gamma, with K = 0) or `--k auto` (K, with gamma = 0): the weight is chosen first (fft_gpu::chooseRegularisation on the same
// mean, with the PSF of the run; --reg names the method -- default gcv for gamma, discrepancy for K -- and --sigma the noise level of the
// discrepancy principle, else estimated), printed as `regularisation: K k gamma g sigma s method m flags f`, and the run then goes on
// exactly as `--k k --cls g` would (`--cls 0` is the Wiener filter).  It combines with `auto auto`.
// `defocus <radius>` in place of length and angle: the PSF is the uniform disk of that radius (diskBlurKernel), and every leg and option
// works as with a motion PSF.  `defocus auto`: the radius is estimated first (fft_gpu::estimateDefocusBlur on the same mean), printed as
// `estimate: defocus radius R diameter D confidence C`, and the run then goes on exactly as `./gpu <img-path> defocus R` would.
// `auto auto --any-blur`: both blurs are looked for in one cepstrum (fft_gpu::estimateBlur), printed as `estimate: kind motion length L
// angle A confidence C` or `estimate: kind defocus radius R diameter D confidence C`, and the run goes on as `L A` or `defocus R` would;
// `estimate: kind none ...` ends the run with a message and a non-zero exit code.  `defocus` beside `blind` is refused with a message.
// `blind <size>` in place of length and angle, with --rl n: the PSF is not stated but refined from a size x size Gaussian start
// (--psf-sigma s, default size / 4) by blind Richardson-Lucy on the per-pixel mean of B, G and R (fft_gpu::richardsonLucyBlind_RGB; --free-boundary,
// --mask and --psf-hold h apply), printed as `blind: size S iterations n psf-sum 1 psf-peak P at (i, j)`; --psf-out file writes the
// PSF min-max scaled.  The Wiener legs of the run then use the refined PSF, and the written result is the blind call's.
// `--rl auto`: the iteration count is found first (fft_gpu::richardsonLucyAuto_RGB on the same mean, with the PSF, form and mask of the run: at most
// --rl-max steps (default 100), stopped by --rl-stop residual (default; --sigma = the noise level of the mean, else estimated) or kl (--gain = photons
// per unit, required), looked at every --rl-check steps), printed as `rl: iterations k of n rule r sigma s statistic v target t stopped 0|1`,
// and the run then goes on exactly as `--rl k` would.  It combines with --accel, --free-boundary, --mask and `auto auto`.
// `--rl n --free-boundary --frame <img2> <L2> <A2> [--frame ...] [--rl-tv lambda [--rl-tv-eps e]] [--mask mask.png]`: the --rl leg is
// fft_gpu::richardsonLucyFrames_RGB -- the picture and every --frame picture (at most 7, all of the picture's size) are exposures of ONE
// scene, each with its own motion PSF (length, angle), restored jointly; --mask serves every frame.  With --register [--max-shift s] the frames
// need not be registered to each other: every frame's translation against the picture is estimated with the PSFs (fft_gpu::RegisterOptions; search
// range s pixels, default min(rows, cols) / 4), printed as `shift: frame k dy .. dx .. confidence ..` and folded into the frame's PSF before the
// restoration.  Beside --frame only --rl n, --free-boundary, --rl-tv, --rl-tv-eps, --mask, --register, --max-shift, --out and --raw-out may stand: anything else (--accel, `--rl auto`, blind, defocus, `auto auto`, --tile, --rl-tv-color,
// --tv, --cls, --k, --sigma, --reg, --norm, --pad, --mode, --host-epilogue, ...) is refused with the usage text, before a picture is read.
// `--rl n --rl-tv lambda [--rl-tv-eps e]`: the --rl leg runs Richardson-Lucy with a total-variation prior of weight lambda (fft_gpu::richardsonLucyTV_RGB;
// eps smooths |grad u|, default FDR_RLTV_EPS); --free-boundary and --mask apply, `auto auto` works as before; --accel, `--rl auto` and `blind` have no
// regularised form and are refused with a message.  The three channels go through one batched call; --rl-tv-color beside --rl-tv couples them
// under one vectorial TV prior (an edge falls in the same place in every channel); without --rl-tv it is a usage error.
// Drop-in counterpart of the reference's gpu.cpp (argument meaning, printed lines and exit codes as at
// gpu.cpp:57-138 of the reference): read image, /255, PSF, K = 0.01, split BGR, warm-up call, timed
// wienerDeblur_RGB_optimized, timed wienerDeblur_RGB_naive, merge, Lab white balance, 8-bit result.
// The serial leg the original runs first (gpu.cpp:83-91) is here too, through the same names (autoPadToPowerOfTwo ->
// fft_serial::wienerDeblur_myfft -> crop): in this repository fft_serial:: runs on the GPU in the parity mode, whose
// pixels are bit-identical to ./serial (tests/), so both "[Speedup]" lines divide that leg's time by a GPU entry
// point's, as gpu.cpp:105,113 do.  There is no CPU code path in this binary.
#include "utils.hpp"
#include "fft/fft.hpp"
#include "fdr_image_io.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <string>

// gpu.cpp:13-55 of the reference: L-inf <= epsilon per channel, else PSNR >= 30 dB still passes ("floating point
// drift").  The reference compares serial vs GPU with it (call commented out at gpu.cpp:116-121); --verify runs it on
// the serial leg's planes (parity mode: the serial path's pixels) against this run's planes: epsilon 1e-4, the
// tolerance BASELINE states.  What it proves is that the two MODES of this library agree; that the parity mode equals
// ./serial is the business of tests/ (against the CPU oracle), and the message says so.
static bool areChannelsEqual(const vector<Mat>& vec1, const vector<Mat>& vec2, double epsilon = 1e-4) {
    if (vec1.size() != vec2.size()) { cerr << "Error: Channel count mismatch.\n"; return false; }
    for (size_t i = 0; i < vec1.size(); ++i) {
        const Mat &m1 = vec1[i], &m2 = vec2[i];
        if (m1.rows != m2.rows || m1.cols != m2.cols || m1.type() != m2.type()) { cerr << "Error: Size/Type mismatch.\n"; return false; }
        double diff = 0.0, sq = 0.0;
        for (int r = 0; r < m1.rows; ++r)
            for (int c = 0; c < m1.cols; ++c) {
                const double d = (double)m1.ptr<float>(r)[c] - (double)m2.ptr<float>(r)[c];
                diff = std::max(diff, std::fabs(d));
                sq += d * d;
            }
        const double mse = sq / ((double)m1.rows * m1.cols);
        const double psnr = mse > 1e-10 ? 10.0 * log10(1.0 / mse) : 100.0;
        if (diff > epsilon) {
            if (psnr >= 30.0) {
                cout << "[Info] Channel " << i << " has floating point drift."
                     << "\n       Max Diff: " << diff << "\n       PSNR: " << psnr << " dB (Excellent! > 30dB is good)"
                     << "\n       -> Verification PASSED (Relaxed)." << endl;
            } else {
                cerr << "[Error] Content mismatch in channel " << i << ".\n";
                cerr << "       Max pixel difference: " << diff << " (Threshold: " << epsilon << ")\n";
                cerr << "       PSNR: " << psnr << " dB (Too low!)\n";
                return false;
            }
        }
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n";
        return -1;
    }
    string img_path = argv[1];
    const bool estimate = string(argv[2]) == "auto" && string(argv[3]) == "auto";
    const bool blind = string(argv[2]) == "blind";  // argv[3] is the PSF's size
    bool defocus = string(argv[2]) == "defocus";    // argv[3] is the disk's radius, or `auto`
    const bool defocus_auto = defocus && string(argv[3]) == "auto";
    if (!estimate && !defocus && (string(argv[2]) == "auto" || string(argv[3]) == "auto")) { cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n"; return -1; }
    int psf_length = estimate || defocus ? 0 : atoi(argv[blind ? 3 : 2]);
    double psf_angle = estimate || blind || defocus ? 0.0 : atof(argv[3]);
    double psf_radius = defocus && !defocus_auto ? atof(argv[3]) : 0.0;
    bool any_blur = false;  // --any-blur, with `auto auto`: motion or defocus, whichever the picture shows
    for (int i = 3; i < argc; ++i)
        if ((defocus && string(argv[i]) == "blind") || (blind && string(argv[i]) == "defocus")) {
            cout << "defocus states the PSF, blind refines one from a Gaussian start: they cannot be combined\n";
            return -1;
        }
    string out_path, raw_path, psf_out_path;  // --psf-out file (blind)
    int psf_hold = 0;                          // --psf-hold h (blind)
    double psf_sigma = 0.0;                    // --psf-sigma s (blind)
    bool blind_opts = false;
    bool verify = false;         // --verify: areChannelsEqual(parity-mode result, this run's result)
    bool host_epilogue = false;  // Lab white balance on the host (the A/B reference of the device epilogue)
    int rl_iterations = -1;      // --rl n: a timed Richardson-Lucy leg after the naive one; its planes are the written result
    bool rl_auto = false;        // --rl auto: the count is found from the picture first
    int rl_max = 100, rl_check = 0;  // --rl-max n, --rl-check c
    string rl_stop;              // --rl-stop residual|kl
    float rl_gain = 0.f;         // --gain g
    bool rl_auto_opts = false;   // one of the four above was given
    bool accel = false;          // --accel: the --rl leg runs the accelerated iteration (vector extrapolation)
    float rl_tv = -1.f, rl_tv_eps = 0.f;  // --rl-tv lambda: the --rl leg is fft_gpu::richardsonLucyTV_RGB; --rl-tv-eps e
    bool rl_tv_opts = false, rl_tv_color = false;  // --rl-tv-color: the channels under one vectorial TV prior (coupled)
    bool free_boundary = false;  // --free-boundary: the --rl leg is fft_gpu::richardsonLucyFree_RGB (the picture is a crop of a larger scene)
    string mask_path;            // --mask file: pixels that are 0 in it (any channel counts) get weight 0, the others weight 1
    struct FrameArg { string path; int length; double angle; };
    vector<FrameArg> frame_args;  // --frame img L A: a further exposure of the same scene with its own motion PSF (fft_gpu::richardsonLucyFrames_RGB)
    bool register_frames = false;  // --register beside --frame: the frames are registered against the picture before the joint restoration
    int max_shift = 0;             // --max-shift s: the search range of --register in pixels (0: min(rows, cols) / 4)
    bool max_shift_set = false;
    int tile = 0, tile_overlap = -1;  // --tile T [--overlap O]: the free-boundary --rl n / --tv mu leg is fft_gpu::restoreTiled_RGB (default O = T / 8)
    float tv_mu = -1.f, tv_rho = 2.0f;  // --tv mu: a timed total-variation leg (fft_gpu::tvDeblur_RGB); its planes are the written result
    int tv_iterations = 50;
    bool tv_opts = false;
    bool tv_color = false;  // --tv-color: vectorial TV, the three channels under one shrinkage (tvDeblur_RGB's coupled form)
    bool tv_auto = false;   // --tv auto: the TV leg is fft_gpu::tvDeblurAuto_RGB, mu chosen from the noise level (--sigma, else estimated)
    float tv_tau = 0.f;     // --tv-tau t: the discrepancy ball is t sigma^2 S (default 1)
    bool tv_tau_given = false, tv_iters_given = false;
    bool poisson = false;       // --poisson: the --tv mu leg is fft_gpu::tvDeblurPoisson_RGB (Poisson likelihood; implies --free-boundary)
    float background = 0.f;     // --background b: the known level under the counts, in the units of the picture (default 0)
    bool background_given = false;
    bool cls = false, parity = false, pad_smooth = false;
    bool cls_auto = false, k_auto = false;  // --cls auto / --k auto: the weight is chosen from the picture
    string reg_method;                      // --reg gcv|discrepancy
    float reg_sigma = 0.f, K = 0.01f;       // --sigma s; --k K
    for (int i = 4; i < argc; ++i) {
        string a = argv[i];
        if (a == "--out" && i + 1 < argc) out_path = argv[++i];
        else if (a == "--raw-out" && i + 1 < argc) raw_path = argv[++i];  // restored float planes B,G,R before white balance
        else if (a == "--host-epilogue") host_epilogue = true;
        else if (a == "--verify") verify = true;
        else if (a == "--any-blur") any_blur = true;
        else if (a == "--mode" && i + 1 < argc) {
            parity = string(argv[++i]) == "parity";
            fft_gpu::set_mode(parity ? FDR_MODE_PARITY : FDR_MODE_FAST);
        }
        else if (a == "--norm" && i + 1 < argc) fft_gpu::set_norm_area(string(argv[++i]) == "cropped" ? FDR_NORM_CROPPED : FDR_NORM_PADDED);
        // constrained least-squares filter (fdr_set_psf_cls) in the fft_gpu:: entry points; the serial leg keeps the Wiener filter.
        // Fast mode only: with --mode parity the library refuses it and the first fft_gpu:: call exits with its message
        else if (a == "--cls" && i + 1 < argc) {
            cls = true;
            if (string(argv[++i]) == "auto") cls_auto = true;
            else fft_gpu::set_cls_gamma(strtof(argv[i], nullptr));
        }
        // the Wiener constant of every leg (default 0.01), or `auto`
        else if (a == "--k" && i + 1 < argc) {
            if (string(argv[++i]) == "auto") k_auto = true;
            else K = strtof(argv[i], nullptr);
        }
        else if (a == "--reg" && i + 1 < argc) reg_method = argv[++i];
        else if (a == "--sigma" && i + 1 < argc) reg_sigma = strtof(argv[++i], nullptr);
        // smooth padding (FDR_OPT_PAD_MODE) in the fft_gpu:: Wiener / CLS entry points; the serial leg keeps zero padding.  Fast mode only:
        // with --mode parity the library refuses it and the first fft_gpu:: call exits with its message
        else if (a == "--pad" && i + 1 < argc) {
            const string v = argv[++i];
            if (v != "zero" && v != "smooth") { cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n"; return -1; }
            pad_smooth = v == "smooth";
            fft_gpu::set_pad_mode(pad_smooth ? FDR_PAD_SMOOTH : FDR_PAD_ZERO);
        }
        // Richardson-Lucy (fft_gpu::richardsonLucy_RGB, fast mode): n >= 0 iterations
        else if (a == "--rl" && i + 1 < argc) {
            if (string(argv[++i]) == "auto") { rl_auto = true; rl_iterations = 0; }
            else rl_iterations = atoi(argv[i]);
        }
        else if (a == "--rl-max" && i + 1 < argc) { rl_auto_opts = true; rl_max = atoi(argv[++i]); }
        else if (a == "--rl-stop" && i + 1 < argc) { rl_auto_opts = true; rl_stop = argv[++i]; }
        else if (a == "--gain" && i + 1 < argc) { rl_auto_opts = true; rl_gain = strtof(argv[++i], nullptr); }
        else if (a == "--rl-check" && i + 1 < argc) { rl_auto_opts = true; rl_check = atoi(argv[++i]); }
        else if (a == "--accel") accel = true;
        else if (a == "--rl-tv" && i + 1 < argc) { rl_tv_opts = true; rl_tv = strtof(argv[++i], nullptr); }
        else if (a == "--rl-tv-eps" && i + 1 < argc) { rl_tv_opts = true; rl_tv_eps = strtof(argv[++i], nullptr); }
        else if (a == "--rl-tv-color") { rl_tv_opts = true; rl_tv_color = true; }
        else if (a == "--free-boundary") free_boundary = true;
        else if (a == "--mask" && i + 1 < argc) mask_path = argv[++i];
        else if (a == "--frame" && i + 3 < argc) { frame_args.push_back({argv[i + 1], atoi(argv[i + 2]), atof(argv[i + 3])}); i += 3; }
        else if (a == "--register") register_frames = true;
        else if (a == "--max-shift" && i + 1 < argc) { max_shift = atoi(argv[++i]); max_shift_set = true; }
        else if (a == "--tile" && i + 1 < argc) tile = atoi(argv[++i]);
        else if (a == "--overlap" && i + 1 < argc) tile_overlap = atoi(argv[++i]);
        else if (a == "--psf-hold" && i + 1 < argc) { blind_opts = true; psf_hold = atoi(argv[++i]); }
        else if (a == "--psf-sigma" && i + 1 < argc) { blind_opts = true; psf_sigma = atof(argv[++i]); }
        else if (a == "--psf-out" && i + 1 < argc) { blind_opts = true; psf_out_path = argv[++i]; }
        // total-variation deconvolution (fft_gpu::tvDeblur_RGB, fast mode): mu > 0, n >= 0 iterations, penalty rho > 0
        else if (a == "--tv" && i + 1 < argc) {
            if (string(argv[++i]) == "auto") tv_auto = true;
            else tv_mu = strtof(argv[i], nullptr);
        }
        else if (a == "--tv-tau" && i + 1 < argc) { tv_tau_given = true; tv_tau = strtof(argv[++i], nullptr); }
        else if (a == "--tv-iters" && i + 1 < argc) { tv_opts = true; tv_iters_given = true; tv_iterations = atoi(argv[++i]); }
        else if (a == "--tv-rho" && i + 1 < argc) { tv_opts = true; tv_rho = strtof(argv[++i], nullptr); }
        else if (a == "--tv-color") { tv_opts = true; tv_color = true; }
        else if (a == "--poisson") poisson = true;
        else if (a == "--background" && i + 1 < argc) { background_given = true; background = strtof(argv[++i], nullptr); }
        else { cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n"; return -1; }
    }
    if (defocus && !defocus_auto && !(psf_radius > 0.0 && psf_radius <= 127.0)) { cout << "Usage: ./gpu <img-path> defocus <radius in (0, 127]|auto>\n"; return -1; }
    if (any_blur && !estimate) { cout << "Usage: ./gpu <img-path> auto auto --any-blur\n"; return -1; }
    // --poisson belongs to --tv mu and is a free-boundary leg of its own: no --tv auto, --rl, --cls, --tile or parity mode beside it;
    // --background belongs to it and is finite and >= 0
    if (poisson || background_given) {
        if (!poisson || !(tv_mu > 0.f) || tv_auto || rl_iterations >= 0 || cls || tile != 0 || tile_overlap != -1 || parity || !(background >= 0.f) ||
            !std::isfinite(background)) {
            cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle> --tv <mu> --poisson [--background b] [--tv-iters n] [--tv-rho r] [--mask m.png] "
                    "[--tv-color] (no --tv auto, --rl, --cls, --tile or --mode parity)\n";
            return -1;
        }
        free_boundary = true;
    }
    // one weight is searched at a time; --reg and --sigma belong to a search
    if ((cls_auto && k_auto) || (!(cls_auto || k_auto) && (!reg_method.empty() || (reg_sigma != 0.f && !rl_auto && !tv_auto))) ||
        (!reg_method.empty() && reg_method != "gcv" && reg_method != "discrepancy") || !(K >= 0.f) || !(reg_sigma >= 0.f)) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n";
        return -1;
    }
    // the RL leg replaces the result the other options shape (CLS filter, parity check, parity-mode restoration)
    if (rl_iterations >= 0 && (cls || verify || parity || pad_smooth)) { cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n"; return -1; }
    // --verify compares against the zero-padded serial leg
    if (pad_smooth && verify) { cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n"; return -1; }
    // --free-boundary belongs to --rl or --tv, --accel to --rl, --mask to --free-boundary (--tv auto is a free-boundary leg with or without the word)
    if ((free_boundary && rl_iterations < 0 && !(tv_mu > 0.f) && !tv_auto) || (accel && rl_iterations < 0) ||
        (!mask_path.empty() && !free_boundary && !tv_auto)) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n";
        return -1;
    }
    // --register belongs to --frame, --max-shift (a range of at least one pixel) to --register
    if ((register_frames && frame_args.empty()) || (max_shift_set && (!register_frames || max_shift < 1))) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle> --rl <n> --free-boundary --frame <img2> <L2> <A2> [--frame ...] --register "
                "[--max-shift <s >= 1>]\n";
        return -1;
    }
    // --frame belongs to --rl n --free-boundary with stated motion PSFs, and takes only --rl-tv, --rl-tv-eps, --mask and --register beside them
    if (!frame_args.empty()) {
        bool ok = rl_iterations >= 0 && free_boundary && !rl_auto && !accel && !blind && !defocus && !estimate && tile == 0 && tile_overlap == -1 &&
                  !rl_tv_color && tv_mu == -1.f && !tv_auto && !poisson && !cls && !cls_auto && !k_auto && !pad_smooth && !parity && !verify &&
                  (int)frame_args.size() < FDR_MAX_FRAMES && psf_length >= 1;
        for (const FrameArg& f : frame_args) ok = ok && f.length >= 1;
        // nothing else beside them: only the words below (with their values) and the two output paths may stand on the command line
        for (int i = 4; i < argc && ok; ++i) {
            const string a = argv[i];
            if (a == "--frame") i += 3;
            else if (a == "--rl" || a == "--rl-tv" || a == "--rl-tv-eps" || a == "--mask" || a == "--out" || a == "--raw-out" || a == "--max-shift") i += 1;
            else ok = a == "--free-boundary" || a == "--register";
        }
        if (!ok) {
            cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle> --rl <n> --free-boundary --frame <img2> <L2> <A2> [--frame ...] [--rl-tv lambda] "
                    "[--mask m.png] [--register [--max-shift s]] (at most 7 --frame; no other leg or option beside them)\n";
            return -1;
        }
    }
    // --tile belongs to the free-boundary form of --rl n or --tv mu, plain: sectioning has no accelerated, TV-prior, data-stopped or blind form
    if (tile != 0 || tile_overlap != -1) {
        if (tile < 1 || !free_boundary || accel || rl_tv_opts || rl_auto || tv_auto || tv_color || blind || (tile_overlap != -1 && (tile_overlap < 0 || tile_overlap > tile / 2))) {
            cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle> --rl <n>|--tv <mu> --free-boundary --tile <T> [--overlap <O in 0 .. T/2>] [--mask m.png]\n";
            return -1;
        }
        if (tile_overlap == -1) tile_overlap = tile / 8;
    }
    // --rl-tv belongs to --rl n; lambda in [0, FDR_RLTV_MAX_LAMBDA], eps finite and >= 0; the prior has no accelerated, data-stopped or blind form
    if (rl_tv_opts) {
        if (accel || rl_auto || blind) {
            cout << "--rl-tv has no accelerated, data-stopped or blind form: it cannot be combined with --accel, --rl auto or blind\n";
            return -1;
        }
        if (rl_iterations < 0 || !(rl_tv >= 0.f && rl_tv <= FDR_RLTV_MAX_LAMBDA) || !(rl_tv_eps >= 0.f) || !std::isfinite(rl_tv_eps)) {
            cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n";
            return -1;
        }
    }
    // --rl-max, --rl-stop, --gain and --rl-check belong to --rl auto; the kl rule needs its gain, the residual rule takes none
    const bool rl_kl = rl_stop == "kl";
    if ((rl_auto_opts && !rl_auto) || (!rl_stop.empty() && rl_stop != "residual" && !rl_kl) || rl_max < 0 || rl_check < 0 ||
        (rl_auto && (rl_kl ? !(rl_gain > 0.f) || reg_sigma != 0.f : rl_gain != 0.f))) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n";
        return -1;
    }
    // blind needs --rl n (a count, plain iteration) and a size; its options belong to it
    if ((blind && (rl_iterations < 0 || rl_auto || accel || psf_length < 1 || psf_length > 256 || psf_hold < 0 || !(psf_sigma >= 0.0) || cls_auto || k_auto)) ||
        (!blind && blind_opts)) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n";
        return -1;
    }
    // so does the TV leg; --tv-iters / --tv-rho / --tv-color belong to --tv, and one run has one iterative leg
    const bool tv = tv_mu > 0.f || tv_auto;
    if ((tv && (cls || verify || parity || pad_smooth || rl_iterations >= 0 || tv_iterations < 0 || !(tv_rho > 0.f))) || (!tv && (tv_opts || tv_mu != -1.f))) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle>\n";
        return -1;
    }
    // --tv auto states no mu and runs the channels one after the other; --tv-tau belongs to it and is >= 0
    if ((tv_auto && (tv_mu != -1.f || tv_color || !(tv_tau >= 0.f) || !std::isfinite(tv_tau))) || (!tv_auto && tv_tau_given)) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle> --tv auto [--sigma s] [--tv-tau t] [--tv-iters n] [--tv-rho r] [--mask m.png] (no --tv-color)\n";
        return -1;
    }
    if (tv_auto && !tv_iters_given) tv_iterations = 100;  // the constrained iteration needs about a hundred steps
    // the free-boundary TV leg runs the channels one after the other: it has no vectorial form
    if (tv && free_boundary && tv_color && !poisson) {
        cout << "Usage: ./gpu <img-path> <psf-length> <psf-angle> --tv <mu> --free-boundary [--mask m.png] [--tv-iters n] [--tv-rho r] (no --tv-color)\n";
        return -1;
    }

    Mat img = fdr_io::imread(img_path);
    if (img.empty()) { cout << "Cannot read image\n"; return -1; }
    img.convertTo(img, CV_32F);
    img /= 255.0;

    Mat gray;  // the per-pixel mean of B, G and R: what the blur and the regularisation weight are found on
    if (estimate || defocus_auto || cls_auto || k_auto || rl_auto) {
        vector<Mat> bgr;
        split(img, bgr);
        gray = Mat(img.rows, img.cols, CV_32F);
        for (int r = 0; r < img.rows; ++r)
            for (int c = 0; c < img.cols; ++c)
                gray.ptr<float>(r)[c] = (bgr[0].ptr<float>(r)[c] + bgr[1].ptr<float>(r)[c] + bgr[2].ptr<float>(r)[c]) / 3.0f;
    }
    fdr_motion_estimate est{};
    fdr_defocus_estimate dest{};
    if (any_blur) {  // the kind of blur and its parameters from one cepstrum
        const fft_gpu::BlurEstimate b = fft_gpu::estimateBlur(gray);
        est = b.motion;
        dest = b.defocus;
        if (b.kind == FDR_BLUR_NONE) {
            printf("estimate: kind none motion-confidence %.3f defocus-confidence %.3f\n", (double)est.confidence, (double)dest.confidence);
            cout << "The picture shows neither a motion blur nor a defocus blur: nothing to restore\n";
            return -1;
        }
        defocus = b.kind == FDR_BLUR_DEFOCUS;
        if (defocus) printf("estimate: kind defocus radius %.17g diameter %d confidence %.3f\n", dest.radius, dest.diameter, (double)dest.confidence);
        else printf("estimate: kind motion length %d angle %.17g confidence %.3f\n", est.length, est.angle_deg, (double)est.confidence);
        fflush(stdout);
        if (defocus) psf_radius = dest.radius;
        else { psf_length = est.length; psf_angle = est.angle_deg; }
    } else if (defocus_auto) {  // the disk's radius from the picture itself
        dest = fft_gpu::estimateDefocusBlur(gray);
        if (dest.diameter < 1) { cout << "Cannot estimate the blur of an all-zero picture\n"; return -1; }
        printf("estimate: defocus radius %.17g diameter %d confidence %.3f\n", dest.radius, dest.diameter, (double)dest.confidence);
        fflush(stdout);
        if (dest.confidence < (float)FDR_DEFOCUS_CONF_MIN)
            cerr << "[Warning] low confidence (" << dest.confidence << " < " << FDR_DEFOCUS_CONF_MIN
                 << "): the picture shows no clear defocus ring; the estimate may be wrong\n";
        psf_radius = dest.radius;
    } else if (estimate) {  // the blur from the picture itself
        est = fft_gpu::estimateMotionBlur(gray);
        if (est.length < 1) { cout << "Cannot estimate the blur of an all-zero picture\n"; return -1; }
        printf("estimate: length %d angle %.17g confidence %.3f\n", est.length, est.angle_deg, (double)est.confidence);
        fflush(stdout);
        if (est.confidence < 10.f)
            cerr << "[Warning] low confidence (" << est.confidence << " < 10): the picture shows no clear motion blur; the estimate may be wrong\n";
        psf_length = est.length;
        psf_angle = est.angle_deg;
    }

    Mat weights;  // --mask: 0 where the mask is 0 in every channel, else 1
    if (!mask_path.empty()) {
        const Mat mask = fdr_io::imread(mask_path);
        if (mask.empty() || mask.rows != img.rows || mask.cols != img.cols) { cout << "Cannot read mask (it must have the image's size)\n"; return -1; }
        const int cn = mask.channels();  // 8-bit, as read
        weights = Mat(img.rows, img.cols, CV_32F);
        for (int r = 0; r < img.rows; ++r)
            for (int c = 0; c < img.cols; ++c) {
                bool any = false;
                for (int k = 0; k < cn; ++k) any = any || mask.ptr<unsigned char>(r)[c * cn + k] != 0;
                weights.ptr<float>(r)[c] = any ? 1.f : 0.f;
            }
    }

    vector<Mat> blind_planes;  // blind: the restored B, G, R of the blind leg
    Mat psf;
    if (blind) {  // the PSF from the picture, refined from a Gaussian start
        Mat start(psf_length, psf_length, CV_32F);
        if (fdr_psf_gaussian(psf_length, psf_sigma, start.ptr<float>(0)) != FDR_OK) { cerr << "Error: " << fdr_last_error() << "\n"; return -1; }
        split(img, blind_planes);
        fft_gpu::BlindOptions bo;
        bo.free_boundary = free_boundary; bo.psf_hold = psf_hold; bo.weights = weights;
        psf = fft_gpu::richardsonLucyBlind_RGB(blind_planes, start, rl_iterations, bo);
        double sum = 0.0;
        float peak = -1.f, lo = psf.ptr<float>(0)[0];
        int pi = 0, pj = 0;
        for (int r = 0; r < psf.rows; ++r)
            for (int c = 0; c < psf.cols; ++c) {
                const float v = psf.ptr<float>(r)[c];
                sum += v;
                lo = std::min(lo, v);
                if (v > peak) { peak = v; pi = r; pj = c; }
            }
        printf("blind: size %d iterations %d psf-sum %.6g psf-peak %.9g at (%d, %d)\n", psf_length, rl_iterations, sum, (double)peak, pi, pj);
        fflush(stdout);
        if (!psf_out_path.empty()) {  // min-max scaled, grey
            Mat k8(psf.rows, psf.cols, CV_8UC3);
            for (int r = 0; r < psf.rows; ++r)
                for (int c = 0; c < psf.cols; ++c) {
                    const float t = peak > lo ? (psf.ptr<float>(r)[c] - lo) / (peak - lo) : 0.f;
                    const unsigned char g = (unsigned char)std::lround(255.0f * t);
                    for (int k = 0; k < 3; ++k) k8.ptr<unsigned char>(r)[3 * c + k] = g;
                }
            if (!fdr_io::imwrite(psf_out_path, k8)) { cout << "Cannot write " << psf_out_path << "\n"; return -1; }
            cout << "Wrote " << psf_out_path << "\n";
        }
    } else if (defocus) {
        psf = diskBlurKernel(psf_radius);
    } else {
        psf = motionBlurKernel(psf_length, psf_angle);
    }
    if (cls_auto || k_auto) {  // the weight from the picture and the PSF: gamma with K = 0, or K with gamma = 0
        const bool gcv = reg_method.empty() ? cls_auto : reg_method == "gcv";
        const fdr_reg_choice c = fft_gpu::chooseRegularisation(gray, psf, gcv ? FDR_REG_GCV : FDR_REG_DISCREPANCY,
                                                               cls_auto ? FDR_REG_PARAM_GAMMA : FDR_REG_PARAM_K, 0.f, reg_sigma);
        K = cls_auto ? 0.f : (float)c.value;
        const float gamma = cls_auto ? (float)c.value : 0.f;
        printf("regularisation: K %.9g gamma %.9g sigma %.9g method %s flags %d\n", (double)K, (double)gamma, c.sigma, gcv ? "gcv" : "discrepancy",
               c.flags);
        fflush(stdout);
        if (c.flags) cerr << "[Warning] the search ended at the " << (c.flags & FDR_REG_AT_LOW ? "lower" : "upper") << " end of its range\n";
        fft_gpu::set_cls_gamma(gamma);
    }

    if (rl_auto) {  // the iteration count from the picture, the PSF and the noise
        vector<Mat> one(1, gray.clone());
        fft_gpu::RlAutoOptions ao;
        ao.sigma = reg_sigma; ao.gain = rl_gain; ao.check_every = rl_check;
        ao.free_boundary = free_boundary; ao.accelerate = accel; ao.weights = weights;
        const fdr_rl_auto_result r = fft_gpu::richardsonLucyAuto_RGB(one, psf, rl_max, rl_kl ? FDR_RL_STOP_KL : FDR_RL_STOP_RESIDUAL, ao)[0];
        printf("rl: iterations %d of %d rule %s sigma %.9g statistic %.9g target %.9g stopped %d\n", r.iterations_done, rl_max,
               rl_kl ? "kl" : "residual", r.sigma, r.statistic, r.target, r.stopped);
        fflush(stdout);
        if (!r.stopped) cerr << "[Warning] the rule did not fire within " << rl_max << " iterations\n";
        rl_iterations = r.iterations_done;
    }

    vector<Mat> channels;
    split(img, channels);
    vector<Mat> input = channels;

    // serial leg (gpu.cpp:83-91): pad, fft_serial::wienerDeblur_myfft, crop -- prints the accumulated phase block
    // of fft/fft_serial.cpp:249-258 on its third call
    vector<Mat> serial_channels = input;
    auto t_start = high_resolution_clock::now();
    for (int i = 0; i < 3; i++) {
        const Mat padded = autoPadToPowerOfTwo(serial_channels[i]);
        const Mat restored = fft_serial::wienerDeblur_myfft(padded, psf, K);
        serial_channels[i] = restored(Rect(0, 0, img.cols, img.rows)).clone();
    }
    auto t_end = high_resolution_clock::now();
    const double serial_time = getElapsedMs(t_start, t_end);
    cout << "Deblurring 3 channels took(serial): " << serial_time << " ms\n";
    // (what that leg is HERE: fft_serial:: on the GPU in the parity mode, one plan + PSF spectrum per channel, run cold --
    // this binary has no CPU path, so the two [Speedup] ratios below compare GPU parity-mode-cold with GPU fast mode, not a
    // CPU with a GPU as gpu.cpp:105,113 of the reference do)
    cout << "[Note] serial leg = fft_serial:: names on the GPU (parity mode, cold); the speed-up lines divide that leg by a GPU entry point\n";

    fft_gpu::wienerDeblur_RGB_optimized(channels, psf, K);  // warm-up, as gpu.cpp:96 (restores in place)

    channels = input;
    t_start = high_resolution_clock::now();
    fft_gpu::wienerDeblur_RGB_optimized(channels, psf, K);
    t_end = high_resolution_clock::now();
    const double opt_time = getElapsedMs(t_start, t_end);
    cout << "Deblurring 3 channels took(gpu[optimize]): " << opt_time << " ms\n";
    printf("[Speedup] %.2fx ms\n", serial_time / opt_time);

    vector<Mat> naive = input;
    t_start = high_resolution_clock::now();
    fft_gpu::wienerDeblur_RGB_naive(naive, psf, K);
    t_end = high_resolution_clock::now();
    const double naive_time = getElapsedMs(t_start, t_end);
    cout << "Deblurring 3 channels took(gpu): " << naive_time << " ms\n";
    printf("[Speedup] %.2fx ms\n", serial_time / naive_time);

    if (blind) {  // the blind leg's planes are the written result
        channels = blind_planes;
    } else if (rl_iterations >= 0) {  // Richardson-Lucy on the same channels: its planes become the written result
        vector<Mat> rl = input;
        t_start = high_resolution_clock::now();
        if (tile > 0) {
            fft_gpu::TiledOptions to;
            to.method = FDR_TILED_RL_FREE; to.tile = tile; to.overlap = tile_overlap; to.iterations = rl_iterations; to.norm_area = FDR_NORM_CROPPED;
            fft_gpu::restoreTiled_RGB(rl, psf, to, weights);
        }
        else if (!frame_args.empty()) {  // the picture and the --frame pictures jointly: the planes of the joint estimate
            vector<vector<Mat>> frames(1, rl);
            vector<Mat> psfs(1, psf);
            for (const FrameArg& f : frame_args) {
                Mat fi = fdr_io::imread(f.path);
                if (fi.empty() || fi.rows != img.rows || fi.cols != img.cols) { cout << "Cannot read frame " << f.path << " (it must have the image's size)\n"; return -1; }
                fi.convertTo(fi, CV_32F);
                fi /= 255.0;
                vector<Mat> ch;
                split(fi, ch);
                frames.push_back(ch);
                psfs.push_back(motionBlurKernel(f.length, f.angle));
            }
            vector<fdr_frame_shift> shifts;
            fft_gpu::RegisterOptions reg;
            reg.on = register_frames; reg.max_shift = max_shift; reg.shifts = &shifts;
            fft_gpu::richardsonLucyFrames_RGB(frames, psfs, rl_iterations, rl_tv_opts ? rl_tv : 0.f, rl_tv_eps, weights, fft_gpu::defaults(),
                                              FDR_RL_SIGMA, reg);
            for (size_t k = 0; k < shifts.size(); ++k)
                cout << "shift: frame " << k << " dy " << shifts[k].dy << " dx " << shifts[k].dx << " confidence " << shifts[k].confidence << "\n";
            rl = frames[0];
        }
        else if (rl_tv_opts) fft_gpu::richardsonLucyTV_RGB(rl, psf, rl_iterations, rl_tv, rl_tv_eps, free_boundary, weights, rl_tv_color);
        else if (free_boundary) fft_gpu::richardsonLucyFree_RGB(rl, psf, rl_iterations, weights, accel);
        else fft_gpu::richardsonLucy_RGB(rl, psf, rl_iterations, accel);
        t_end = high_resolution_clock::now();
        cout << "Deblurring 3 channels took(gpu[richardson-lucy " << (free_boundary ? "free-boundary " : "") << rl_iterations
             << (accel ? " accelerated" : "");
        if (tile > 0) cout << " tile " << tile << " overlap " << tile_overlap;
        if (!frame_args.empty()) cout << " frames " << frame_args.size() + 1;
        if (rl_tv_opts) cout << " tv " << rl_tv;
        cout << "]): " << getElapsedMs(t_start, t_end) << " ms\n";
        channels = rl;
    }

    if (tv) {  // total-variation deconvolution on the same channels: its planes become the written result
        vector<Mat> tvc = input;
        vector<fdr_tv_auto_result> chosen;
        t_start = high_resolution_clock::now();
        if (tv_auto) chosen = fft_gpu::tvDeblurAuto_RGB(tvc, psf, reg_sigma, tv_iterations, tv_rho, tv_tau, weights);
        else if (tile > 0) {
            fft_gpu::TiledOptions to;
            to.method = FDR_TILED_TV_FREE; to.tile = tile; to.overlap = tile_overlap; to.iterations = tv_iterations; to.mu = tv_mu; to.rho = tv_rho;
            to.norm_area = FDR_NORM_CROPPED;
            fft_gpu::restoreTiled_RGB(tvc, psf, to, weights);
        }
        else if (poisson) fft_gpu::tvDeblurPoisson_RGB(tvc, psf, tv_mu, tv_iterations, tv_rho, weights, background, tv_color);
        else if (free_boundary) fft_gpu::tvDeblurFree_RGB(tvc, psf, tv_mu, tv_iterations, tv_rho, weights);
        else fft_gpu::tvDeblur_RGB(tvc, psf, tv_mu, tv_iterations, tv_rho, tv_color);
        t_end = high_resolution_clock::now();
        for (const fdr_tv_auto_result& r : chosen)
            printf("total-variation: sigma %.9g target %.9g mu %.9g discrepancy %.9g\n", r.sigma, r.target, r.mu, r.discrepancy);
        fflush(stdout);
        cout << "Deblurring 3 channels took(gpu[total-variation " << (poisson ? "poisson " : free_boundary && !tv_auto ? "free-boundary " : "");
        if (tv_auto) cout << "auto";
        else cout << "mu " << tv_mu;
        if (poisson) cout << " background " << background;
        cout << " rho " << tv_rho << " n " << tv_iterations << (tv_color ? " colour" : "");
        if (tile > 0) cout << " tile " << tile << " overlap " << tile_overlap;
        cout << "]): " << getElapsedMs(t_start, t_end) << " ms\n";
        channels = tvc;
    }

    if (verify) {  // the check of gpu.cpp:116-121 between the serial leg's planes and this run's planes
        if (areChannelsEqual(serial_channels, channels))
            cout << "[Success] fast mode matches the serial-equivalent parity mode (L-inf <= 1e-4 per channel, or PSNR >= 30 dB).\n";
        else
            cout << "[Error] fast mode and the serial-equivalent parity mode differ.\n";
    }

    if (!raw_path.empty()) {
        FILE* f = fopen(raw_path.c_str(), "wb");
        if (!f) { cout << "Cannot write " << raw_path << "\n"; return -1; }
        for (const Mat& c : channels)
            for (int r = 0; r < c.rows; ++r) fwrite(c.ptr<float>(r), sizeof(float), (size_t)c.cols, f);
        fclose(f);
    }

    Mat corrected_BGR;
    if (host_epilogue) {  // the reference's sequence on the host (gpu.cpp:123-137)
        Mat merged_float;
        merge(channels, merged_float);
        Mat merged_Lab = fdr_io::bgr2lab(merged_float), img_orig_Lab = fdr_io::bgr2lab(img);
        Mat corrected_Lab = applyWhiteBalance(merged_Lab, img_orig_Lab);
        corrected_BGR = fdr_io::lab2bgr(corrected_Lab);
        corrected_BGR.convertTo(corrected_BGR, CV_8U, 255.0);
    } else {              // the same epilogue in two device passes (fdr_white_balance_u8)
        const float* orig[3]; const float* rest[3];
        vector<Mat> keep_o, keep_r;
        for (int c = 0; c < 3; ++c) {
            keep_o.push_back(input[c].isContinuous() ? input[c] : input[c].clone());
            keep_r.push_back(channels[c].isContinuous() ? channels[c] : channels[c].clone());
        }
        for (int c = 0; c < 3; ++c) { orig[c] = keep_o[c].ptr<float>(0); rest[c] = keep_r[c].ptr<float>(0); }
        corrected_BGR = Mat(img.rows, img.cols, CV_8UC3);
        if (fdr_white_balance_u8(0, orig, rest, img.rows, img.cols, img.cols, corrected_BGR.ptr<unsigned char>(0), 3 * img.cols) != FDR_OK) {
            cerr << "Error: " << __FILE__ << ":" << __LINE__ << ", " << fdr_last_error() << "\n";
            exit(1);
        }
    }
    if (!out_path.empty()) {
        if (!fdr_io::imwrite(out_path, corrected_BGR)) { cout << "Cannot write " << out_path << "\n"; return -1; }
        cout << "Wrote " << out_path << "\n";
    }
    return 0;
}
