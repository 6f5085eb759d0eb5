// TEST PROGRAM: camera edits and many views in one launch through the C++ drop-in header
// (sp_amd::look_at, Scene::set_camera, sp_amd::render_views), compiled and linked the way a host
// program would (g++, -I include, -l simplepath_hip).  tests/test_gpu_views.py runs it and compares
// its images with Python's.
//
//   views_main <scene.sp> --size W H --spp N [--integrator NAME] [--bvh 0|1] --output PREFIX
//              --view ex ey ez  lx ly lz  fov   (twice or more; up is +y)
//
// Writes PREFIX<v>.pfm for every view (one sp_render_views call), then sets the LAST view's camera on
// the scene, renders it with render_image and writes PREFIX_set.pfm.
#include "simplepath_amd.hpp"

#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::cerr << "usage: " << argv[0] << " scene.sp --size W H --spp N [--integrator NAME] [--bvh 0|1] --output PREFIX"
                  << " --view ex ey ez lx ly lz fov [--view ...]\n";
        return EXIT_FAILURE;
    }
    struct View {
        float eye[3], target[3], fov;
    };
    std::string       file_path = argv[1], output = "view", integrator_name = "direct_lighting";
    std::vector<View> views;
    int               bvh = 0, width = 0, height = 0;
    unsigned          spp = 1;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--size" && i + 2 < argc) { width = std::atoi(argv[++i]); height = std::atoi(argv[++i]); }
        else if (a == "--spp" && i + 1 < argc) spp = static_cast<unsigned>(std::atoi(argv[++i]));
        else if (a == "--integrator" && i + 1 < argc) integrator_name = argv[++i];
        else if (a == "--bvh" && i + 1 < argc) bvh = std::atoi(argv[++i]);
        else if (a == "--output" && i + 1 < argc) output = argv[++i];
        else if (a == "--view" && i + 7 < argc) {
            View v{};
            for (float& x : v.eye) x = std::strtof(argv[++i], nullptr);
            for (float& x : v.target) x = std::strtof(argv[++i], nullptr);
            v.fov = std::strtof(argv[++i], nullptr);
            views.push_back(v);
        } else {
            std::cerr << "unknown argument " << a << '\n';
            return EXIT_FAILURE;
        }
    }
    try {
        const sp_amd::Integrator integrator(sp_amd::string_to_integrator_type(integrator_name), SP_PIPELINE_MEGAKERNEL);
        sp_amd::Scene            scene = sp_amd::parse_scene_file(file_path);
        if (width > 0) scene.set_resolution(width, height);
        scene.upload(0, bvh);
        const float                 up[3] = { 0.0f, 1.0f, 0.0f };
        std::vector<sp_camera_desc> cameras;
        for (const View& v : views) cameras.push_back(sp_amd::look_at(v.eye, v.target, up, v.fov, scene.image_width, scene.image_height));
        sp_render_stats                 st{};
        const std::vector<sp_amd::Image> images = sp_amd::render_views(integrator, spp, scene, cameras, &st);
        for (size_t v = 0; v < images.size(); ++v) {
            const std::string name = output + std::to_string(v) + ".pfm";
            sp_amd::check(sp_write_pfm(name.c_str(), images[v].width, images[v].height, images[v].rgb.data()));
        }
        std::cout << "views " << images.size() << " rays " << st.rays << " launches " << st.launches << '\n';
        if (!cameras.empty()) {
            scene.set_camera(cameras.back());
            sp_render_stats     one{};
            const sp_amd::Image img  = sp_amd::render_image(integrator, spp, scene, &one);
            const std::string   name = output + "_set.pfm";
            sp_amd::check(sp_write_pfm(name.c_str(), img.width, img.height, img.rgb.data()));
            std::cout << "set_camera rays " << one.rays << '\n';
        }
    } catch (const sp_amd::ParsingException& e) {
        std::cerr << "ParsingException: " << e.what() << '\n';
        return 2;
    } catch (const std::exception& e) {
        std::cerr << e.what() << '\n';
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
