// pyrite_host_tool -- the BASELINE configurations and the example scenes written against the C++ host surface
// (include/pyrite_host.hpp), the way pyrite_amd/scenes.py writes them against the Python surface.
//
//   pyrite_host_tool dump   <scene> <data_dir> <out.bin>                      flatten only (no GPU): canonical scene bytes + camera + renderer
//   pyrite_host_tool dump-project   <project.lua> <texel dir | -> <out.bin>    the same for a project file (lua_project.cpp)
//   pyrite_host_tool render-project <project.lua> <texel dir | -> <seed> <out.png> [film.bin]   what `pyrite project.lua` does (main.rs:46-330)
//                                   [--size WxH] [--spp N] [--features PREFIX] [--features-grid N] [--hdr PATH] [--exposure EV|auto] [--tone clip|reinhard]
//                                   [--despeckle [K]] [--despeckle-radius R] [--upsample N] [--upsample-radius R] [--glare [STRENGTH]] [--glare-levels N] [--glare-threshold T]
//                                   [--lens-blur] [--lens-blur-radius R] [--build host|device] and the progressive flags of python -m pyrite_amd
//   pyrite_host_tool encode-features <records.bin> <normal.rgb> <depth.rgb>    PyrFeaturePixel[n] -> the 8-bit normal and depth images, raw RGB (no GPU)
//   pyrite_host_tool intersect <scene> <data_dir> <rays.f32> <hits.bin>       World::intersect for a ray batch ([n][6] f32 -> PyrHit[n])
//   pyrite_host_tool render <scene> <data_dir> <w> <h> <spp> <seed> <film.bin> [out.png]
//                                                                             Renderer::render on device 0; film as raw {acc, weight} f32
// scenes: c1 c2 spheres diamonds lamps textures      data_dir: pyrite_amd/data (cornell_spectra.json, cornell_box.obj, diamonds.obj)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <optional>
#include <sstream>

#include "pyrite_host.hpp"

using namespace pyrite;

// {"name": {"format": "array", "min": a, "max": b, "points": [...]}, ...} -- the one shape cornell_spectra.json has
static Expression read_spectrum(const std::string& json, const std::string& name) {
    size_t at = json.find("\"" + name + "\"");
    if (at == std::string::npos) throw ProjectError("spectrum " + name + " not found");
    auto number_after = [&](const char* key) {
        size_t k = json.find(key, at);
        return (float)std::strtod(json.c_str() + k + std::strlen(key), nullptr);
    };
    const float mn = number_after("\"min\":"), mx = number_after("\"max\":");
    size_t k = json.find("\"points\":", at);
    k = json.find('[', k) + 1;
    std::vector<float> points;
    for (;;) {
        char* end = nullptr;
        const double v = std::strtod(json.c_str() + k, &end);
        points.push_back((float)v);
        k = (size_t)(end - json.c_str());
        while (json[k] == ' ' || json[k] == ',') ++k;
        if (json[k] == ']') break;
    }
    return spectrum_array(mn, mx, std::move(points));
}

struct Cornell {
    Material light, white, green, red;
    Expression lamp;
};
static Cornell cornell_materials(const std::string& data_dir) { // pyrite/test/cornell/cornell.lua:4-7, :41-51
    std::ifstream f(data_dir + "/cornell_spectra.json");
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string json = ss.str();
    Cornell c;
    c.lamp = read_spectrum(json, "lamp");
    c.light = Material(material::emissive(c.lamp * 3) + material::diffuse(0.78));
    c.white = Material(material::diffuse(read_spectrum(json, "white")));
    c.green = Material(material::diffuse(read_spectrum(json, "green")));
    c.red = Material(material::diffuse(read_spectrum(json, "red")));
    return c;
}
static CameraProject cornell_camera() { // cornell.lua:28-35
    CameraProject cam;
    cam.fov = 37.7;
    cam.transform = transform::look_at(vector(-2.78, -8.0, 2.73), vector(-2.78, 0, 2.73), vector(0, 0, 1));
    return cam;
}

static Project scene_c1(const std::string& data_dir) { // scenes.py c1_spheres
    const Cornell m = cornell_materials(data_dir);
    const double R = 100.0, x0 = -5.56, x1 = 0.0, y1 = 5.592, z0 = 0.0, z1 = 5.488;
    const double cx = (x0 + x1) / 2, cy = y1 / 2, cz = (z0 + z1) / 2;
    Project p;
    p.camera = cornell_camera();
    p.world.objects = {
        Sphere{vector(x0 - R, cy, cz), R, m.red, {}},   Sphere{vector(x1 + R, cy, cz), R, m.green, {}}, Sphere{vector(cx, y1 + R, cz), R, m.white, {}},
        Sphere{vector(cx, cy, z0 - R), R, m.white, {}}, Sphere{vector(cx, cy, z1 + R), R, m.white, {}}, Sphere{vector(-3.7, 3.3, 0.9), 0.9, m.white, {}},
        Sphere{vector(-1.6, 1.7, 0.8), 0.8, m.white, {}},
        Sphere{vector(-2.78, 2.795, 4.9), 0.5, Material(material::emissive(cornell_materials(data_dir).lamp * 3)), {}},
    };
    return p;
}

static Project scene_c2(const std::string& data_dir) { // scenes.py c2_cornell: test/cornell/box.obj, materials per cornell.lua:41-51
    const Cornell m = cornell_materials(data_dir);
    Mesh mesh;
    mesh.file = data_dir + "/cornell_box.obj";
    mesh.materials = {{"light", m.light}, {"left", m.red},     {"right", m.green}, {"tall", m.white},
                      {"short", m.white}, {"back", m.white},   {"ceiling", m.white}, {"floor", m.white}};
    Project p;
    p.camera = cornell_camera();
    p.world.objects = {mesh};
    return p;
}

static Project scene_spheres() { // pyrite/test/spheres/spheres.lua:1-69
    const Expression green = spectrum_curve({{400, 0}, {450, 0.3f}, {500, 0}, {550, 1}, {600, 0}});
    const Expression red = spectrum_curve({{580, 0}, {600, 1}, {610, 1}, {650, 0}});
    Project p;
    p.camera.fov = 53;
    p.camera.transform = transform::look_at(vector(0, 1, 0), vector(0, 1, 1));
    p.renderer.spectrum_samples = 10, p.renderer.tile_size = 32, p.renderer.light_samples = 4;
    p.world.objects = {
        Sphere{vector(0, -50, 10), 50.0, Material(material::diffuse(1)), {}},
        Sphere{vector(0, 1.5, 10), 1.5, Material(material::emissive(light_source::d65() * 3)), {}},
        Sphere{vector(-3, 1.4, 10), 1.5, Material(mix(material::mirror(1), material::diffuse(green), fresnel(1.5))), {}},
        Sphere{vector(3, 1.4, 10), 1.5, Material(material::diffuse(red)), {}},
    };
    return p;
}

static Project scene_diamonds(const std::string& data_dir) { // pyrite/test/diamonds/diamonds.lua:1-60
    Mesh mesh;
    mesh.file = data_dir + "/diamonds.obj";
    mesh.materials = {
        {"diamonds", Material(material::refractive(1, 2.37782, Expression(0.01371)))},
        {"light_left", Material(material::emissive(light_source::d65()))},
        {"light_right", Material(material::emissive(light_source::d65() * 2))},
        {"bottom", Material(material::mirror(mix(Expression(0), Expression(0.2), fresnel(1.1))))},
    };
    Project p;
    p.renderer.spectrum_samples = 1, p.renderer.tile_size = 32, p.renderer.bounces = 32;
    p.camera.fov = 12.5;
    p.camera.focus_distance = 11.08, p.camera.aperture = 0.02;
    p.camera.transform = transform::look_at(vector(-6.55068, -8.55076, 4.0), vector(0.1, 0, 0.1), vector(0, 0, 1));
    p.world.objects = {mesh};
    return p;
}

static Project scene_lamps() { // scenes.py lamps_example: the lamp kinds and opcodes no other scene reaches
    Project p;
    p.renderer.light_samples = 2, p.renderer.bounces = 6, p.renderer.tile_size = 16;
    p.camera.fov = 45;
    p.camera.transform = transform::look_at(vector(0, -7, 2.5), vector(0, 0, 0.8), vector(0, 0, 1));
    p.world.sky = light_source::d65() * 0.2;
    p.world.objects = {
        Plane{vector(0, 0, 0), vector(0, 0, 1), Material(material::diffuse(0.5)), {}},
        Sphere{vector(-1.2, 0, 1), 1.0, Material(material::refractive(1, 1.5)), {}},
        Sphere{vector(1.2, 0.5, 0.7), 0.7, Material(material::diffuse(blackbody(3000) * 2e-13)), {}},
        Sphere{vector(0.2, -1.6, 0.5), 0.5, Material(material::diffuse(rgb(0.8, 0.3, 0.1))), {}},
        PointLight{vector(3, -3, 5), light_source::d65() * 40},
        DirectionalLight{vector(-0.3, 0.2, 0.933), 0.98, light_source::a() * 2},
    };
    return p;
}

// scenes.py textures_example: colour / mono textures and normal maps on all three shape kinds, a uv-mapped mesh held in memory
// with scale + transform, a textured lamp. The 16 x 16 texel arrays (already linear f32, what Texture::from_path leaves in
// memory) are read from <data_dir>/<name>.f32, written there by the test from the same generated images.
static std::vector<float> read_floats(const std::string& path, size_t count) {
    std::ifstream f(path, std::ios::binary);
    std::vector<float> v(count);
    if (!f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * 4))) throw ProjectError("could not read " + path);
    return v;
}
static Project scene_textures(const std::string& dir) {
    const uint32_t n = 16;
    const Expression checker = color_texture(n, n, read_floats(dir + "/checker.f32", n * n * 4));
    const Expression nmap = color_texture(n, n, read_floats(dir + "/nmap_linear.f32", n * n * 4));
    const Expression rgba = color_texture(n, n, read_floats(dir + "/rgba.f32", n * n * 4));
    const Expression mono_linear = mono_texture(n, n, read_floats(dir + "/mono_linear.f32", n * n));
    const Expression mono_srgb = mono_texture(n, n, read_floats(dir + "/mono_srgb.f32", n * n));
    auto quad = std::make_shared<MeshData>();
    quad->position = {-1.5f, 1.0f, 0.2f, 0.5f, 1.0f, 0.2f, 0.5f, 2.6f, 1.4f, -1.5f, 2.6f, 1.4f};
    quad->texture = {0, 0, 2, 0, 2, 1.5f, 0, 1.5f};
    quad->normal = {0, -0.6f, 0.8f, 0.1f, -0.6f, 0.8f, 0, -0.55f, 0.83f, -0.1f, -0.6f, 0.8f};
    quad->objects = {MeshData::Object{"quad", {{{0, 0, 0}, {1, 1, 1}, {2, 2, 2}}, {{0, 0, 0}, {2, 2, 2}, {3, 3, 3}}}}};
    Mesh mesh;
    mesh.data = quad;
    mesh.transform = transform::look_at(vector(0.3, 0.2, 0), vector(0.3, 0.2, -1), vector(0.1, 1, 0));
    mesh.scale = 1.1;
    mesh.materials = {{"quad", Material(material::diffuse(checker), nmap)}};
    Project p;
    p.renderer.light_samples = 2, p.renderer.bounces = 5, p.renderer.tile_size = 16, p.renderer.spectrum_samples = 6;
    p.camera.fov = 50;
    p.camera.transform = transform::look_at(vector(0, -6, 2.6), vector(0, 0, 0.8), vector(0, 0, 1));
    p.world.sky = light_source::d65() * 0.15;
    p.world.objects = {
        Plane{vector(0, 0, 0), vector(0, 0, 1), Material(material::diffuse(checker * 0.9), nmap), vector(1.5, 2.5)},
        Sphere{vector(-1.6, -0.4, 0.9), 0.9, Material(material::diffuse(rgba), nmap), vector(0.25, 0.5)},
        Sphere{vector(1.5, 0.2, 0.7), 0.7, Material(mix(material::mirror(1), material::diffuse(rgb(0.9, 0.8, 0.3)), mono_linear)), {}},
        mesh,
        Sphere{vector(0.2, -1.4, 2.6), 0.35, Material(material::emissive(light_source::d65() * mono_srgb * 25)), vector(0.5, 0.5)},
        PointLight{vector(3, -3, 4), light_source::a() * 6},
    };
    return p;
}

static Project make_scene(const std::string& name, const std::string& data_dir) {
    if (name == "textures") return scene_textures(data_dir);
    if (name == "c1") return scene_c1(data_dir);
    if (name == "c2") return scene_c2(data_dir);
    if (name == "spheres") return scene_spheres();
    if (name == "diamonds") return scene_diamonds(data_dir);
    if (name == "lamps") return scene_lamps();
    throw ProjectError("unknown scene " + name);
}

// Texels for project files: <dir>/<file name>.<linear|srgb>.<mono|color>.f32 = u32 width, u32 height, f32 texels (already
// linear) -- written by whoever decodes the images (tests: pyrite_amd/images.py).
static TextureLoader texel_files(const std::string& dir) {
    return [dir](const std::string& path, bool linear, bool mono, uint32_t& width, uint32_t& height) {
        const size_t slash = path.find_last_of('/');
        const std::string file = dir + "/" + path.substr(slash == std::string::npos ? 0 : slash + 1) + (linear ? ".linear" : ".srgb") + (mono ? ".mono" : ".color") + ".f32";
        std::ifstream f(file, std::ios::binary);
        uint32_t wh[2] = {0, 0};
        if (!f.read(reinterpret_cast<char*>(wh), 8)) throw ProjectError("could not load " + path + " (no " + file + ")");
        width = wh[0], height = wh[1];
        std::vector<float> texels((size_t)width * height * (mono ? 1 : 4));
        if (!f.read(reinterpret_cast<char*>(texels.data()), (std::streamsize)(texels.size() * 4))) throw ProjectError("short texel file " + file);
        return texels;
    };
}

static void write_dump(const char* path, FlatScene& flat, const Project& project) {
    const PyrSceneDesc& d = flat.desc();
    std::vector<uint8_t> bytes(pyrh_serialize_desc(&d, nullptr, 0));
    pyrh_serialize_desc(&d, bytes.data(), bytes.size());
    const Camera cam = Camera::from_project(project.camera);
    const Renderer r = Renderer::from_project(project.renderer);
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(bytes.data()), (std::streamsize)bytes.size());
    f.write(reinterpret_cast<const char*>(&cam.c), sizeof(cam.c));
    const uint32_t params[8] = {r.bounces, r.pixel_samples, r.light_samples, r.spectrum_samples, r.spectrum_bins, r.tile_size, project.image.width, project.image.height};
    f.write(reinterpret_cast<const char*>(params), sizeof(params));
    std::printf("%zu scene bytes, %zu triangles, %zu spheres, %zu planes\n", bytes.size(), flat.num_triangles(), flat.num_spheres(), flat.num_planes());
}

int main(int argc, char** argv) {
    try {
        if (argc >= 5 && std::string(argv[1]) == "dump-project") { // dump-project <project.lua> <texel dir | -> <out.bin>
            const LoadedProject loaded = load_project(argv[2], std::string(argv[3]) == "-" ? TextureLoader() : texel_files(argv[3]));
            FlatScene flat;
            flat.add_world(loaded.project.world, loaded.base_dir);
            write_dump(argv[4], flat, loaded.project);
            return 0;
        }
        if (argc >= 6 && std::string(argv[1]) == "render-project") { // render-project <project.lua> <texel dir | -> <seed> <out.png> [film.bin] [--pass-samples N] [--preview PATH] [--preview-every SECONDS] [--noise] [--despeckle [K]] [--despeckle-radius R] [--denoise] [--denoise-radius N] [--upsample N] [--upsample-radius R] [--glare [STRENGTH]] [--glare-levels N] [--glare-threshold T] [--lens-blur] [--lens-blur-radius R] [--build host|device]
            // the flags of python -m pyrite_amd: a progressive session with previews (main.rs:261-299) instead of one blocking call
            std::optional<long> pass_samples;
            std::string preview_path, film_path;
            double preview_every = 20.0; // main.rs:262
            bool noise = false;
            std::string features_prefix, size;
            std::optional<long> features_grid, spp;
            std::optional<std::string> hdr, exposure, tone_name;
            bool denoise_flag = false;
            std::optional<long> denoise_radius;
            std::optional<std::string> despeckle_k; // --despeckle [K]: the next argument unless it is a flag, as --glare reads its strength
            std::optional<long> despeckle_radius;
            std::optional<long> upsample_scale, upsample_radius; // --upsample N: the render at 1/N of the image size, the final image upsampled to it
            std::optional<std::string> glare_strength; // --glare [STRENGTH]: the next argument unless it is a flag, as argparse's nargs="?" reads it (a film path goes before it)
            std::optional<long> glare_levels;
            std::optional<double> glare_threshold;
            bool lens_blur_flag = false; // --lens-blur: the frame through a pinhole, the project camera's lens applied by the filter over the feature records
            std::optional<long> lens_blur_radius;
            std::optional<std::string> build_name; // --build host|device: who builds the BVH; given, the stage times go to stderr
            for (int i = 6; i < argc; ++i) {
                const std::string a = argv[i];
                auto value = [&]() -> const char* {
                    if (i + 1 >= argc) throw ProjectError(a + " needs a value");
                    return argv[++i];
                };
                if (a == "--pass-samples")
                    pass_samples = std::strtol(value(), nullptr, 10);
                else if (a == "--preview")
                    preview_path = value();
                else if (a == "--preview-every")
                    preview_every = std::strtod(value(), nullptr);
                else if (a == "--noise")
                    noise = true;
                else if (a == "--features")
                    features_prefix = value();
                else if (a == "--features-grid")
                    features_grid = std::strtol(value(), nullptr, 10);
                else if (a == "--hdr")
                    hdr = value();
                else if (a == "--exposure")
                    exposure = value();
                else if (a == "--tone")
                    tone_name = value();
                else if (a == "--denoise")
                    denoise_flag = true;
                else if (a == "--denoise-radius")
                    denoise_radius = std::strtol(value(), nullptr, 10);
                else if (a == "--despeckle")
                    despeckle_k = i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0 ? argv[++i] : "6.0";
                else if (a == "--despeckle-radius")
                    despeckle_radius = std::strtol(value(), nullptr, 10);
                else if (a == "--upsample")
                    upsample_scale = std::strtol(value(), nullptr, 10);
                else if (a == "--upsample-radius")
                    upsample_radius = std::strtol(value(), nullptr, 10);
                else if (a == "--glare")
                    glare_strength = i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0 ? argv[++i] : "0.1";
                else if (a == "--glare-levels")
                    glare_levels = std::strtol(value(), nullptr, 10);
                else if (a == "--glare-threshold")
                    glare_threshold = std::strtod(value(), nullptr);
                else if (a == "--lens-blur")
                    lens_blur_flag = true;
                else if (a == "--lens-blur-radius")
                    lens_blur_radius = std::strtol(value(), nullptr, 10);
                else if (a == "--build")
                    build_name = value();
                else if (a == "--size")
                    size = value();
                else if (a == "--spp")
                    spp = std::strtol(value(), nullptr, 10);
                else if (a.rfind("--", 0) == 0)
                    throw ProjectError("unknown flag " + a);
                else
                    film_path = a;
            }
            std::string problem = progressive_flag_problem(pass_samples, !preview_path.empty(), preview_every, noise);
            if (problem.empty()) problem = features_flag_problem(!features_prefix.empty(), features_grid);
            if (problem.empty()) problem = tone_flag_problem(hdr, exposure, tone_name);
            if (problem.empty()) problem = despeckle_flag_problem(despeckle_k, despeckle_radius);
            if (problem.empty()) problem = denoise_flag_problem(denoise_flag, denoise_radius);
            if (problem.empty()) problem = upsample_flag_problem(upsample_scale, upsample_radius);
            if (problem.empty()) problem = glare_flag_problem(glare_strength, glare_levels, glare_threshold);
            if (problem.empty()) problem = lens_blur_flag_problem(lens_blur_flag, lens_blur_radius);
            if (problem.empty() && build_name && *build_name != "host" && *build_name != "device") problem = "--build takes host or device";
            if (!problem.empty()) {
                std::fprintf(stderr, "error: %s\n", problem.c_str());
                return 2;
            }
            const std::optional<PyrToneParams> tone = tone_from_flags(exposure, tone_name);
            const std::optional<PyrGlareParams> glare_p = glare_from_flags(glare_strength, glare_levels, glare_threshold);
            const std::optional<PyrDespeckleParams> despeckle_p = despeckle_from_flags(despeckle_k, despeckle_radius);
            const std::optional<PyrUpsampleParams> upsample_p = upsample_from_flags(upsample_scale, upsample_radius);
            LoadedProject loaded = load_project(argv[2], std::string(argv[3]) == "-" ? TextureLoader() : texel_files(argv[3]));
            if (!size.empty()) { // WIDTHxHEIGHT, as python -m pyrite_amd --size
                char* rest = nullptr;
                loaded.project.image.width = (uint32_t)std::strtoul(size.c_str(), &rest, 10);
                loaded.project.image.height = (uint32_t)std::strtoul(rest && *rest ? rest + 1 : "0", nullptr, 10);
            }
            if (spp && *spp > 0) loaded.project.renderer.pixel_samples = (uint32_t)*spp;
            problem = despeckle_flag_problem(despeckle_k, despeckle_radius, loaded.project.renderer.pixel_samples, pass_samples);
            if (problem.empty()) problem = denoise_flag_problem(denoise_flag, denoise_radius, loaded.project.renderer.pixel_samples, pass_samples);
            const uint32_t full_width = loaded.project.image.width, full_height = loaded.project.image.height;
            if (problem.empty()) problem = upsample_flag_problem(upsample_scale, upsample_radius, full_width, full_height);
            if (!problem.empty()) {
                std::fprintf(stderr, "error: %s\n", problem.c_str());
                return 2;
            }
            if (upsample_p) // the render and everything before the upsample at 1/N of the size, under the same camera
                loaded.project.image.width = full_width / (uint32_t)*upsample_scale, loaded.project.image.height = full_height / (uint32_t)*upsample_scale;
            const Project& project = loaded.project;
            std::unique_ptr<World> world = World::from_project(project.world, loaded.base_dir);
            const Camera lens_cam = Camera::from_project(project.camera);
            Camera cam = lens_cam;
            if (lens_blur_flag) cam.c.aperture = 0.0f; // the render, its guides and every filter before the lens see a pinhole
            Renderer r = Renderer::from_project(project.renderer);
            r.seed = std::strtoull(argv[4], nullptr, 10);
            Film film = r.new_film(project.image.width, project.image.height);
            std::printf("The scene contains %zu objects.\n", world->num_objects()); // world.rs:251-254
            if (build_name) {
                world->scene(0, 0, *build_name == "device" ? World::Build::Device : World::Build::Host);
                const PyrBuildInfo b = world->build_info(0);
                std::fprintf(stderr, "build: asked %s, used %s (fallback %u), %u levels, %u median splits, digest %016llx; bounds %.2f tree %.2f finish %.2f collapse %.2f pack+upload %.2f total %.2f ms\n",
                             build_name->c_str(), b.builder_used == PYR_BUILD_DEVICE ? "device" : "host", b.fallback_reason, b.levels, b.median_splits, (unsigned long long)b.tree_digest,
                             b.bounds_ms, b.tree_ms, b.finish_ms, b.collapse_ms, b.pack_upload_ms, b.total_ms);
            }
            std::vector<float> linear;
            if (pass_samples || !preview_path.empty() || noise || denoise_flag || despeckle_p) {
                const uint32_t per_pass = pass_samples ? (uint32_t)*pass_samples : denoise_flag || despeckle_p ? r.pixel_samples / 2u : kDefaultPassSamples;
                Session session(r, film.width, film.height, cam, *world, noise || denoise_flag || despeckle_p);
                auto last_image = std::chrono::steady_clock::now(); // main.rs:241
                while (session.samples_done() < r.pixel_samples) {
                    session.render(per_pass);
                    session.sync();
                    std::printf("Rendering... %3d %%\n", (int)((uint64_t)session.samples_done() * 100u / r.pixel_samples));
                    if (!preview_path.empty() && std::chrono::duration<double>(std::chrono::steady_clock::now() - last_image).count() >= preview_every) {
                        save_png(preview_path,
                                 tone ? session.preview_tone(*tone, 30.0f, project.image.filter, project.image.white) : session.preview(30.0f, project.image.filter, project.image.white),
                                 film.width, film.height);
                        std::printf("Preview updated (%u samples per pixel)\n", session.samples_done());
                        if (noise && session.samples_done() >= 2 * per_pass) {
                            std::vector<float> tiles = session.noise();
                            std::sort(tiles.begin(), tiles.end());
                            const size_t n = tiles.size();
                            const float median = n % 2 ? tiles[n / 2] : 0.5f * (tiles[n / 2 - 1] + tiles[n / 2]);
                            std::printf("noise: largest tile %.4g, median tile %.4g\n", tiles.back(), median);
                        }
                        last_image = std::chrono::steady_clock::now();
                    }
                }
                if (despeckle_p) { // the halves cleaned, then the denoiser or their mean
                    const std::optional<PyrDenoiseParams> denoise_p = denoise_flag ? std::optional<PyrDenoiseParams>(denoise_params(denoise_radius ? (uint32_t)*denoise_radius : PYR_DENOISE_RADIUS)) : std::nullopt;
                    DespeckledImage cleaned = session.despeckled(*despeckle_p, denoise_p, true, 2.0f, project.image.filter, project.image.white);
                    std::printf("despeckle: %u pixels clamped in half A, %u in half B\n", cleaned.counts[0], cleaned.counts[1]);
                    linear = std::move(cleaned.image);
                } else if (denoise_flag)
                    linear = session.denoised(denoise_params(denoise_radius ? (uint32_t)*denoise_radius : PYR_DENOISE_RADIUS), true, 2.0f, project.image.filter, project.image.white).image;
                film = session.film();
            } else {
                r.render(film, cam, *world);
            }
            std::printf("Saving final result...\n"); // main.rs:313
            if (!denoise_flag && !despeckle_p && (hdr || tone || glare_p || upsample_p || lens_blur_flag)) linear = develop_linear(film, PYR_LINEAR_SRGB, project.image.filter, project.image.white);
            if (upsample_p) { // after the denoiser, before the glare
                const Features low_guides = r.features(film.width, film.height, cam, *world), guides = r.features(full_width, full_height, cam, *world);
                const std::vector<float> low_albedo = develop_linear(low_guides.albedo, PYR_LINEAR_SRGB, project.image.filter, project.image.white);
                const std::vector<float> albedo = develop_linear(guides.albedo, PYR_LINEAR_SRGB, project.image.filter, project.image.white);
                linear = upsample(linear, film.width, film.height, (uint32_t)*upsample_scale, *upsample_p, &albedo, &guides.pixels, &low_albedo, &low_guides.pixels);
            }
            if (lens_blur_flag) // after the filters that read the guides, before the glare and the tone curve; the full-size records
                linear = lens_blur(linear, r.features(full_width, full_height, cam, *world).pixels, full_width, full_height,
                                   lens_blur_params(lens_cam, lens_blur_radius ? (uint32_t)*lens_blur_radius : PYR_LENS_BLUR_MAX_RADIUS));
            if (glare_p) linear = glare(linear, full_width, full_height, *glare_p); // before the statistics of an automatic exposure, which tonemap takes
            save_png(argv[5],
                     tone || denoise_flag || despeckle_p || glare_p || upsample_p || lens_blur_flag ? tonemap(linear, full_width, full_height, tone ? *tone : tone_params(PYR_TONE_CLIP, 1.0f))
                                                                    : film.develop(project.image.filter, project.image.white),
                     full_width, full_height);
            if (hdr) {
                write_linear(*hdr, linear, full_width, full_height);
                std::printf("wrote %s\n", hdr->c_str());
            }
            if (!film_path.empty()) {
                std::ofstream f(film_path, std::ios::binary);
                f.write(reinterpret_cast<const char*>(film.grains.data()), (std::streamsize)(film.grains.size() * sizeof(PyrGrain)));
            }
            if (!features_prefix.empty()) {
                write_feature_images(features_prefix, r.features(full_width, full_height, cam, *world, features_grid ? (uint32_t)*features_grid : 1u), project.image.filter,
                                     project.image.white);
                std::printf("wrote %s_albedo.png, %s_normal.png, %s_depth.png\n", features_prefix.c_str(), features_prefix.c_str(), features_prefix.c_str());
            }
            return 0;
        }
        if (argc >= 5 && std::string(argv[1]) == "encode-features") { // encode-features <records.bin> <normal.rgb> <depth.rgb>
            std::ifstream in(argv[2], std::ios::binary);
            std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            std::vector<PyrFeaturePixel> pixels(bytes.size() / sizeof(PyrFeaturePixel));
            std::memcpy(pixels.data(), bytes.data(), pixels.size() * sizeof(PyrFeaturePixel));
            const std::vector<uint8_t> normal = encode_normal_image(pixels), depth = encode_depth_image(pixels);
            std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char*>(normal.data()), (std::streamsize)normal.size());
            std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char*>(depth.data()), (std::streamsize)depth.size());
            return 0;
        }
        if (argc >= 5 && std::string(argv[1]) == "dump") {
            Project project = make_scene(argv[2], argv[3]);
            FlatScene flat;
            flat.add_world(project.world, argv[3]);
            std::printf("%s: ", argv[2]);
            write_dump(argv[4], flat, project);
            return 0;
        }
        if (argc >= 4 && std::string(argv[1]) == "objects") { // objects <scene> <data_dir>: what moves together (tests)
            Project project = make_scene(argv[2], argv[3]);
            std::unique_ptr<World> world = World::from_project(project.world, argv[3]);
            for (const FlatScene::Object& o : world->objects())
                std::printf("%s %u %u %u %u\n", o.name.c_str(), o.range.first_triangle, o.range.num_triangles, o.range.first_sphere, o.range.num_spheres);
            return 0;
        }
        if (argc >= 6 && std::string(argv[1]) == "pose") { // pose <scene> <data_dir> <poses.f32: 17 floats an object> <geometry.f32> [rebuild] (tests)
            Project project = make_scene(argv[2], argv[3]);
            std::unique_ptr<World> world = World::from_project(project.world, argv[3]);
            std::ifstream in(argv[4], std::ios::binary);
            std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            if (bytes.size() != world->objects().size() * 17 * 4) throw ProjectError("pose: the file does not hold 17 floats for each of the scene's objects");
            std::map<size_t, World::ObjectPose> poses;
            for (size_t k = 0; k < world->objects().size(); ++k) {
                World::ObjectPose pose;
                std::memcpy(pose.transform, bytes.data() + k * 68, 64);
                std::memcpy(&pose.scale, bytes.data() + k * 68 + 64, 4);
                poses[k] = pose;
            }
            world->pose(poses, argc >= 7 && std::string(argv[6]) == "rebuild" ? World::Update::Rebuild : World::Update::Refit);
            const World::Geometry g = world->geometry();
            std::ofstream out(argv[5], std::ios::binary);
            for (const std::vector<float>* a : {&g.positions, &g.normals, &g.frames, &g.spheres}) out.write(reinterpret_cast<const char*>(a->data()), (std::streamsize)(a->size() * 4));
            std::printf("%zu objects posed\n", poses.size());
            return 0;
        }
        if (argc >= 7 && std::string(argv[1]) == "skin") { // skin <scene> <data_dir> <bindings> <joints.f32> <geometry.f32> [refit|rebuild [dual_quaternion]] (tests)
            // bindings: u32 object, num_joints; u16 joints[T][3][4]; f32 weights[T][3][4] for the object's T triangles. joints.f32: 16 floats a joint.
            Project project = make_scene(argv[2], argv[3]);
            std::unique_ptr<World> world = World::from_project(project.world, argv[3]);
            const auto slurp = [](const char* path) {
                std::ifstream in(path, std::ios::binary);
                return std::vector<char>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            };
            const std::vector<char> bindings = slurp(argv[4]), table = slurp(argv[5]);
            uint32_t head[2] = {0, 0};
            if (bindings.size() < 8) throw ProjectError("skin: the bindings file is too short");
            std::memcpy(head, bindings.data(), 8);
            if (head[0] >= world->objects().size()) throw ProjectError("skin: no such object");
            const size_t words = 12 * (size_t)world->objects()[head[0]].range.num_triangles;
            if (bindings.size() != 8 + words * 6) throw ProjectError("skin: the bindings file does not hold the object's triangles");
            if (table.size() != (size_t)head[1] * 64) throw ProjectError("skin: the joints file does not hold 16 floats for each joint");
            World::Skin skin;
            skin.num_joints = head[1];
            if (argc >= 9 && std::string(argv[8]) == "dual_quaternion") skin.blend = PYR_SKIN_DUAL_QUATERNION;
            skin.joints.resize(words), skin.weights.resize(words);
            if (words) std::memcpy(skin.joints.data(), bindings.data() + 8, words * 2), std::memcpy(skin.weights.data(), bindings.data() + 8 + words * 2, words * 4);
            std::vector<float> joints(table.size() / 4);
            if (!joints.empty()) std::memcpy(joints.data(), table.data(), table.size());
            world->set_skins({{head[0], skin}});
            world->skin({{head[0], joints}}, nullptr, argc >= 8 && std::string(argv[7]) == "rebuild" ? World::Update::Rebuild : World::Update::Refit);
            const World::Geometry g = world->geometry();
            std::ofstream out(argv[6], std::ios::binary);
            for (const std::vector<float>* a : {&g.positions, &g.normals, &g.frames, &g.spheres}) out.write(reinterpret_cast<const char*>(a->data()), (std::streamsize)(a->size() * 4));
            std::printf("object %u skinned to %u joints\n", head[0], head[1]);
            return 0;
        }
        if (argc >= 7 && std::string(argv[1]) == "morph") { // morph <scene> <data_dir> <targets> <weights.f32> <geometry.f32> [rebuild] (tests)
            // targets: u32 object, num_targets, has_normals; f32 position_deltas[num_targets][T][3][3]; f32 normal_deltas of the same
            // shape if has_normals, for the object's T triangles. weights.f32: one float a target.
            Project project = make_scene(argv[2], argv[3]);
            std::unique_ptr<World> world = World::from_project(project.world, argv[3]);
            const auto slurp = [](const char* path) {
                std::ifstream in(path, std::ios::binary);
                return std::vector<char>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            };
            const std::vector<char> targets = slurp(argv[4]), table = slurp(argv[5]);
            uint32_t head[3] = {0, 0, 0};
            if (targets.size() < 12) throw ProjectError("morph: the targets file is too short");
            std::memcpy(head, targets.data(), 12);
            if (head[0] >= world->objects().size()) throw ProjectError("morph: no such object");
            const size_t words = 9 * (size_t)world->objects()[head[0]].range.num_triangles * head[1];
            if (targets.size() != 12 + words * 4 * (head[2] ? 2 : 1)) throw ProjectError("morph: the targets file does not hold the object's triangles");
            if (table.size() != (size_t)head[1] * 4) throw ProjectError("morph: the weights file does not hold one float for each target");
            World::Morph morph;
            morph.num_targets = head[1];
            morph.position_deltas.resize(words);
            if (words) std::memcpy(morph.position_deltas.data(), targets.data() + 12, words * 4);
            if (head[2]) {
                morph.normal_deltas.resize(words);
                if (words) std::memcpy(morph.normal_deltas.data(), targets.data() + 12 + words * 4, words * 4);
            }
            std::vector<float> weights(table.size() / 4);
            if (!weights.empty()) std::memcpy(weights.data(), table.data(), table.size());
            world->set_morphs({{head[0], morph}});
            world->morph({{head[0], weights}}, nullptr, nullptr, argc >= 8 && std::string(argv[7]) == "rebuild" ? World::Update::Rebuild : World::Update::Refit);
            const World::Geometry g = world->geometry();
            std::ofstream out(argv[6], std::ios::binary);
            for (const std::vector<float>* a : {&g.positions, &g.normals, &g.frames, &g.spheres}) out.write(reinterpret_cast<const char*>(a->data()), (std::streamsize)(a->size() * 4));
            std::printf("object %u morphed over %u targets\n", head[0], head[1]);
            return 0;
        }
        if (argc >= 7 && std::string(argv[1]) == "smooth") { // smooth <scene> <data_dir> <labels> <pose.f32> <geometry.f32> [rebuild] (tests)
            // labels: u32 object, has_labels; u32 vertex_ids[T][3] for the object's T triangles if has_labels, else the object is
            // welded by its rest positions and normals. pose.f32: transform[16] column-major and the scale, for that object.
            Project project = make_scene(argv[2], argv[3]);
            std::unique_ptr<World> world = World::from_project(project.world, argv[3]);
            const auto slurp = [](const char* path) {
                std::ifstream in(path, std::ios::binary);
                return std::vector<char>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            };
            const std::vector<char> labels = slurp(argv[4]), posed = slurp(argv[5]);
            uint32_t head[2] = {0, 0};
            if (labels.size() < 8) throw ProjectError("smooth: the labels file is too short");
            std::memcpy(head, labels.data(), 8);
            if (head[0] >= world->objects().size()) throw ProjectError("smooth: no such object");
            const size_t corners = 3 * (size_t)world->objects()[head[0]].range.num_triangles;
            if (labels.size() != 8 + (head[1] ? corners * 4 : 0)) throw ProjectError("smooth: the labels file does not hold the object's corners");
            if (posed.size() != 17 * 4) throw ProjectError("smooth: the pose file does not hold 17 floats");
            std::vector<uint32_t> ids(head[1] ? corners : 0);
            if (!ids.empty()) std::memcpy(ids.data(), labels.data() + 8, corners * 4);
            World::ObjectPose pose;
            std::memcpy(pose.transform, posed.data(), 64);
            std::memcpy(&pose.scale, posed.data() + 64, 4);
            world->set_smoothing({{head[0], ids}});
            world->pose({{head[0], pose}}, argc >= 8 && std::string(argv[7]) == "rebuild" ? World::Update::Rebuild : World::Update::Refit);
            const World::Geometry g = world->geometry();
            std::ofstream out(argv[6], std::ios::binary);
            for (const std::vector<float>* a : {&g.positions, &g.normals, &g.frames, &g.spheres}) out.write(reinterpret_cast<const char*>(a->data()), (std::streamsize)(a->size() * 4));
            std::printf("object %u smoothed over %zu corners\n", head[0], corners);
            return 0;
        }
        if (argc >= 6 && std::string(argv[1]) == "intersect") { // intersect <scene> <data_dir> <rays.f32> <hits.bin>
            Project project = make_scene(argv[2], argv[3]);
            std::unique_ptr<World> world = World::from_project(project.world, argv[3]);
            std::ifstream in(argv[4], std::ios::binary);
            std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            std::vector<float> rays(bytes.size() / 4);
            std::memcpy(rays.data(), bytes.data(), rays.size() * 4);
            const std::vector<PyrHit> hits = world->intersect(rays);
            std::ofstream out(argv[5], std::ios::binary);
            out.write(reinterpret_cast<const char*>(hits.data()), (std::streamsize)(hits.size() * sizeof(PyrHit)));
            std::printf("%zu rays\n", hits.size());
            return 0;
        }
        if (argc >= 9 && std::string(argv[1]) == "render") {
            Project project = make_scene(argv[2], argv[3]);
            project.image.width = (uint32_t)std::atoi(argv[4]), project.image.height = (uint32_t)std::atoi(argv[5]);
            project.renderer.pixel_samples = (uint32_t)std::atoi(argv[6]);
            std::unique_ptr<World> world = World::from_project(project.world, argv[3]);
            const Camera cam = Camera::from_project(project.camera);
            Renderer r = Renderer::from_project(project.renderer);
            r.seed = std::strtoull(argv[7], nullptr, 10);
            Film film = r.new_film(project.image.width, project.image.height);
            std::printf("The scene contains %zu objects.\n", world->num_objects()); // world.rs:251-254
            int last = -1;
            auto report = [&](Progress p) {
                if (p.progress != last) std::printf("%s... %3d %%\n", p.message, (int)p.progress);
                last = p.progress;
            };
            if (const char* list = std::getenv("PYRITE_DEVICES")) { // e.g. 0,1,2,3 -- Renderer::render over several GPUs
                std::vector<int> devices;
                for (const char* c = list; *c;) {
                    devices.push_back((int)std::strtol(c, const_cast<char**>(&c), 10));
                    if (*c == ',') ++c;
                }
                r.render(film, cam, *world, devices, report);
            } else {
                r.render(film, cam, *world, report);
            }
            std::ofstream f(argv[8], std::ios::binary);
            f.write(reinterpret_cast<const char*>(film.grains.data()), (std::streamsize)(film.grains.size() * sizeof(PyrGrain)));
            std::printf("film weight %.0f\n", film.total_weight());
            if (argc >= 10) {
                const std::vector<uint8_t> rgb = film.develop(project.image.filter, project.image.white);
                save_png(argv[9], rgb, film.width, film.height);
                std::printf("wrote %s\n", argv[9]);
            }
            return 0;
        }
        std::fprintf(stderr, "usage: pyrite_host_tool dump <scene> <data_dir> <out.bin> | render <scene> <data_dir> <w> <h> <spp> <seed> <film.bin> [out.png]\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
