// TEST PROGRAM: a resumable render through the C++ drop-in header (sp_amd::ProgressiveRender),
// compiled and linked the way a host program would (g++, -I include, -l simplepath_hip).
// tests/test_progress_dropin.py runs it: the passes' image must be the one-shot image bit for bit.
//
//   progressive_main <scene.sp> --passes N[,N...] [--integrator NAME] [--bvh 0|1] [--size W H] --output FILE
//                    [--checkpoint]   (export after the first pass, continue in a second object)
#include "simplepath_amd.hpp"

#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::cerr << "usage: " << argv[0] << " scene.sp --passes N[,N...] [--integrator NAME] [--bvh 0|1] [--size W H]"
                  << " --output FILE [--checkpoint]\n";
        return EXIT_FAILURE;
    }
    std::string           file_path = argv[1], output = "progressive.pfm", integrator_name = "direct_lighting";
    std::vector<unsigned> passes;
    int                   bvh = 0, width = 0, height = 0;
    bool                  checkpoint = false;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--passes" && i + 1 < argc) {
            std::stringstream ss(argv[++i]);
            std::string       tok;
            while (std::getline(ss, tok, ',')) passes.push_back(static_cast<unsigned>(std::atoi(tok.c_str())));
        } else if (a == "--integrator" && i + 1 < argc) integrator_name = argv[++i];
        else if (a == "--bvh" && i + 1 < argc) bvh = std::atoi(argv[++i]);
        else if (a == "--size" && i + 2 < argc) { width = std::atoi(argv[++i]); height = std::atoi(argv[++i]); }
        else if (a == "--output" && i + 1 < argc) output = argv[++i];
        else if (a == "--checkpoint") checkpoint = true;
        else {
            std::cerr << "unknown argument " << a << '\n';
            return EXIT_FAILURE;
        }
    }
    try {
        const sp_amd::IntegratorType type = sp_amd::string_to_integrator_type(integrator_name);
        sp_amd::Scene                scene = sp_amd::parse_scene_file(file_path);
        if (width > 0) scene.set_resolution(width, height);
        scene.upload(0, bvh);
        sp_amd::ProgressiveRender prog(scene, type);
        unsigned long long        rays = 0;
        for (size_t k = 0; k < passes.size(); ++k) {
            rays += prog.render_more(passes[k]).rays;
            if (checkpoint && k == 0) { // a second object continues from the first one's state
                unsigned                   n  = 0;
                std::vector<sp_pixel_state> st = prog.export_state(&n);
                sp_amd::ProgressiveRender  next(scene, type);
                next.import_state(st, n);
                prog = std::move(next);
            }
        }
        const sp_amd::Image img = prog.image();
        sp_amd::check(sp_write_pfm(output.c_str(), img.width, img.height, img.rgb.data()));
        std::cout << "wrote " << output << " (" << img.width << "x" << img.height << ", " << prog.samples() << " spp in "
                  << passes.size() << " passes, " << rays << " rays)\n";
    } catch (const sp_amd::ParsingException& e) {
        std::cerr << "ParsingException: " << e.what() << '\n';
        return 2;
    } catch (const std::exception& e) {
        std::cerr << e.what() << '\n';
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
