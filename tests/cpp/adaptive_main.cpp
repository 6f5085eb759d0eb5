// TEST PROGRAM: adaptive sampling through the C++ drop-in header (sp_amd::render_adaptive), compiled
// and linked the way a host program would (g++, -I include, -l simplepath_hip).
// tests/test_adaptive_abi.py runs it: image and per-tile counts must be the Python binding's.
//
//   adaptive_main <scene.sp> --rule THRESHOLD MIN MAX STEP [--integrator NAME] [--bvh 0|1] [--size W H]
//                 --output FILE.pfm --counts FILE.u32
#include "simplepath_amd.hpp"

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::cerr << "usage: " << argv[0] << " scene.sp --rule THRESHOLD MIN MAX STEP [--integrator NAME] [--bvh 0|1]"
                  << " [--size W H] --output FILE.pfm --counts FILE.u32\n";
        return EXIT_FAILURE;
    }
    std::string file_path = argv[1], output = "adaptive.pfm", counts = "adaptive.u32", integrator_name = "direct_lighting";
    int         bvh = 0, width = 0, height = 0;
    float       threshold = 0.05f;
    unsigned    lo = 1, hi = 16, step = 4;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--rule" && i + 4 < argc) {
            threshold = static_cast<float>(std::atof(argv[++i]));
            lo        = static_cast<unsigned>(std::atoi(argv[++i]));
            hi        = static_cast<unsigned>(std::atoi(argv[++i]));
            step      = static_cast<unsigned>(std::atoi(argv[++i]));
        } else if (a == "--integrator" && i + 1 < argc) integrator_name = argv[++i];
        else if (a == "--bvh" && i + 1 < argc) bvh = std::atoi(argv[++i]);
        else if (a == "--size" && i + 2 < argc) { width = std::atoi(argv[++i]); height = std::atoi(argv[++i]); }
        else if (a == "--output" && i + 1 < argc) output = argv[++i];
        else if (a == "--counts" && i + 1 < argc) counts = argv[++i];
        else {
            std::cerr << "unknown argument " << a << '\n';
            return EXIT_FAILURE;
        }
    }
    try {
        const sp_amd::IntegratorType type  = sp_amd::string_to_integrator_type(integrator_name);
        sp_amd::Scene                scene = sp_amd::parse_scene_file(file_path);
        if (width > 0) scene.set_resolution(width, height);
        scene.upload(0, bvh);
        const sp_amd::Integrator    integrator(type);
        const sp_amd::AdaptiveImage r = sp_amd::render_adaptive(integrator, scene, threshold, lo, hi, step);
        sp_amd::check(sp_write_pfm(output.c_str(), r.image.width, r.image.height, r.image.rgb.data()));
        std::ofstream(counts, std::ios::binary)
            .write(reinterpret_cast<const char*>(r.tile_samples.data()), static_cast<std::streamsize>(r.tile_samples.size() * 4));
        std::cout << "wrote " << output << " (" << r.image.width << "x" << r.image.height << ", " << r.rounds << " rounds, "
                  << r.samples_total << " samples)\n";
    } catch (const sp_amd::ParsingException& e) {
        std::cerr << "ParsingException: " << e.what() << '\n';
        return 2;
    } catch (const std::exception& e) {
        std::cerr << e.what() << '\n';
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
