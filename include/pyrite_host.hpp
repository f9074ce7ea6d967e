// pyrite_host.hpp -- C++ host side above the C ABI of pyrite_gpu.h.
//
// The reference is compiled code (Rust) whose toolchain is absent from this image, so the host layer that mirrors its
// operator surface is C++ (libpyrite_host.so, pyrite_amd/csrc/host/pyrite_host.cpp). It offers, with the reference's names,
// argument meaning and defaults:
//
//   * the project tree the Lua prelude builds               pyrite/src/project/lib.lua:1-309, project/mod.rs:103-252
//       expressions (numbers, vector, rgb, spectrum, blackbody, fresnel, texture, + - * /, mix, clamp, light_source.d65 / a)
//       materials   (emissive, diffuse, mirror, refractive, mix, a + b)
//       objects     (sphere, plane, mesh, directional light, point light), look_at transform, perspective camera
//   * ProgramCompiler::compile                                pyrite/src/program/compiler.rs:48-586 (+ operand coercion :682-968)
//   * SurfaceMaterial::from_project                            pyrite/src/materials/mod.rs:90-227
//   * World::from_project (+ make_triangle, OBJ ingest)        pyrite/src/world.rs:39-271, :308-374
//   * Camera::from_project, Renderer::from_project             pyrite/src/cameras.rs:30-55, renderer/mod.rs:31-75
//   * the seam Renderer::render(film, camera, world)            pyrite/src/renderer/mod.rs:77-111  -> pyr_render_simple
//   * Film (film.rs:9-114) and its development to 8-bit sRGB    pyrite/src/main.rs:190-238, :315-418 -> pyr_film_develop
//
// Nothing here computes radiance: rendering and development are calls into libpyrite_gpu.so, which fails with
// PYR_ERR_DEVICE when no MI355X is present. Errors are reported as pyrite::ProjectError (what the reference reports as a
// project error) or pyrite::GpuError (a non-zero PyrStatus).
#ifndef PYRITE_HOST_HPP
#define PYRITE_HOST_HPP

#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "pyrite_gpu.h"

namespace pyrite {

struct ProjectError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct GpuError : std::runtime_error {
    int status;
    GpuError(int status_, const std::string& what) : std::runtime_error(what), status(status_) {}
};

// ------------------------------------------------------------------------------------------------ expressions
// ComplexExpression / Expression (project/expressions.rs:163-201). A plain number is Expression::Number (f64).
struct ExprNode;
class Expression {
  public:
    Expression(double number = 0.0); // NOLINT: numbers convert implicitly, as in the Lua prelude
    Expression(int number) : Expression((double)number) {}
    explicit Expression(std::shared_ptr<const ExprNode> node) : node_(std::move(node)) {}
    const ExprNode& node() const { return *node_; }
    const ExprNode* id() const { return node_.get(); } // identity: one spectrum / register per Lua table
    bool is_number() const;
    double number() const;
    Expression mix(const Expression& other, const Expression& amount) const;

  private:
    std::shared_ptr<const ExprNode> node_;
};

enum class ExprKind { Number, Vector, Rgb, Spectrum, Fresnel, Blackbody, Binary, Mix, Clamp, ColorTexture, MonoTexture };
enum class BinaryOp { Add, Sub, Mul, Div };
enum class SpectrumFormat { Array, Curve, BuiltinD65, BuiltinA };

struct ExprNode {
    ExprKind kind = ExprKind::Number;
    double number = 0.0;
    BinaryOp op = BinaryOp::Add;
    std::vector<Expression> args; // Vector x y z w | Rgb r g b | Fresnel ior env_ior | Blackbody T | Binary l r | Mix l r amount | Clamp value min max
    // Spectrum (project/spectra.rs:13-24)
    SpectrumFormat format = SpectrumFormat::Array;
    float min = 0.0f, max = 0.0f;
    std::vector<float> points; // Array: values; Curve: (wavelength, value) pairs
    // Textures: linear f32 texels [height][width][channels] (4 for colour, 1 for mono), top row first -- what
    // Texture::from_path leaves in memory (texture.rs:25-85). Decoding image files is the front-end's job.
    uint32_t tex_width = 0, tex_height = 0;
    std::vector<float> texels;
};

Expression operator+(const Expression& a, const Expression& b);
Expression operator-(const Expression& a, const Expression& b);
Expression operator*(const Expression& a, const Expression& b);
Expression operator/(const Expression& a, const Expression& b);
Expression mix(const Expression& lhs, const Expression& rhs, const Expression& amount);             // lib.lua:104-118
Expression clamp(const Expression& value, const Expression& min, const Expression& max);            // expressions.rs:47-63
Expression fresnel(const Expression& ior, const Expression& env_ior = 1.0);                         // lib.lua:120-125
Expression vector(const Expression& x = 0.0, const Expression& y = 0.0, const Expression& z = 0.0, const Expression& w = 0.0); // :128-150
Expression blackbody(const Expression& temperature);                                                // lib.lua:152-157
Expression rgb(const Expression& red = 0.0, const Expression& green = 0.0, const Expression& blue = 0.0); // lib.lua:166-176
Expression spectrum_array(float min, float max, std::vector<float> points);                         // lib.lua:159-164, format = "array"
Expression spectrum_curve(std::vector<std::pair<float, float>> points);                             // format = "curve"
Expression color_texture(uint32_t width, uint32_t height, std::vector<float> rgba_linear);           // lib.lua:178-195
Expression mono_texture(uint32_t width, uint32_t height, std::vector<float> luma_linear);
namespace light_source { // lib.lua:254-258
Expression d65();
Expression a();
} // namespace light_source

// ------------------------------------------------------------------------------------------------ materials
// SurfaceMaterial nodes (project/materials.rs:5-35).
enum class MaterialKind { Emissive, Diffuse, Mirror, Refractive, Mix, Add };
struct MaterialNode;
class SurfaceMaterial {
  public:
    SurfaceMaterial() = default;
    explicit SurfaceMaterial(std::shared_ptr<const MaterialNode> node) : node_(std::move(node)) {}
    const MaterialNode* get() const { return node_.get(); }
    SurfaceMaterial mix(const SurfaceMaterial& other, const Expression& amount) const;

  private:
    std::shared_ptr<const MaterialNode> node_;
};
struct MaterialNode {
    MaterialKind kind = MaterialKind::Diffuse;
    Expression color;
    Expression ior = 1.0;
    std::optional<Expression> dispersion, env_ior, env_dispersion;
    SurfaceMaterial lhs, rhs;
    Expression amount;
};
namespace material { // lib.lua:231-252
SurfaceMaterial diffuse(const Expression& color);
SurfaceMaterial emissive(const Expression& color);
SurfaceMaterial mirror(const Expression& color);
SurfaceMaterial refractive(const Expression& color, const Expression& ior, std::optional<Expression> dispersion = std::nullopt,
                           std::optional<Expression> env_ior = std::nullopt, std::optional<Expression> env_dispersion = std::nullopt);
} // namespace material
SurfaceMaterial operator+(const SurfaceMaterial& a, const SurfaceMaterial& b); // lib.lua:88-90
SurfaceMaterial mix(const SurfaceMaterial& lhs, const SurfaceMaterial& rhs, const Expression& amount);

struct Material { // project::Material: {surface, normal_map}
    SurfaceMaterial surface;
    std::optional<Expression> normal_map;
    Material() = default;
    Material(SurfaceMaterial s) : surface(std::move(s)) {} // NOLINT
    Material(SurfaceMaterial s, Expression n) : surface(std::move(s)), normal_map(std::move(n)) {}
};

// ------------------------------------------------------------------------------------------------ transforms, camera, objects
struct LookAt { // Transform::LookAt, project/mod.rs:243-266
    Expression from = vector(), to = vector();
    std::optional<Expression> up; // default (0, 1, 0)
};
namespace transform {
inline LookAt look_at(Expression from, Expression to, std::optional<Expression> up = std::nullopt) { return LookAt{std::move(from), std::move(to), std::move(up)}; }
} // namespace transform

// The `obj` crate's data model (0.10.2): objects -> polygons of (position, texture?, normal?) index tuples.
struct MeshData {
    struct Index {
        int32_t position = -1, texture = -1, normal = -1; // -1 = absent
    };
    struct Object {
        std::string name;
        std::vector<std::vector<Index>> polys;
    };
    std::vector<float> position; // [n][3]
    std::vector<float> texture;  // [n][2]
    std::vector<float> normal;   // [n][3]
    std::vector<Object> objects;
};
MeshData load_obj(const std::string& path);

struct Sphere {
    Expression position, radius;
    Material material;
    std::optional<Expression> texture_scale;
};
struct Plane {
    Expression origin, normal;
    Material material;
    std::optional<Expression> texture_scale;
};
struct Mesh {
    std::string file;                          // OBJ path, relative to the project directory ...
    std::shared_ptr<const MeshData> data;      // ... or geometry already in memory
    std::map<std::string, Material> materials; // by OBJ object name (world.rs:199-208)
    std::optional<Expression> scale;
    std::optional<LookAt> transform;
};
struct DirectionalLight {
    Expression direction, width, color;
};
struct PointLight {
    Expression position, color;
};
struct WorldObject { // project::WorldObject, project/mod.rs:169-203
    enum class Kind { Sphere, Plane, Mesh, DirectionalLight, PointLight } kind;
    Sphere sphere;
    Plane plane;
    Mesh mesh;
    DirectionalLight directional;
    PointLight point;
    WorldObject(Sphere s) : kind(Kind::Sphere), sphere(std::move(s)) {}                     // NOLINT
    WorldObject(Plane p) : kind(Kind::Plane), plane(std::move(p)) {}                         // NOLINT
    WorldObject(Mesh m) : kind(Kind::Mesh), mesh(std::move(m)) {}                            // NOLINT
    WorldObject(DirectionalLight l) : kind(Kind::DirectionalLight), directional(std::move(l)) {} // NOLINT
    WorldObject(PointLight l) : kind(Kind::PointLight), point(std::move(l)) {}               // NOLINT
};
struct WorldProject { // project::World, project/mod.rs:163-167
    std::optional<Expression> sky;
    std::vector<WorldObject> objects;
};
struct CameraProject { // project::Camera::Perspective, project/mod.rs:120-129
    LookAt transform;
    Expression fov = 45.0;
    std::optional<Expression> focus_distance, aperture;
};
struct RendererProject { // project::Renderer::Simple + RendererShared, project/mod.rs:131-161
    uint32_t pixel_samples = 1;
    std::optional<uint32_t> bounces, light_samples, spectrum_samples, spectrum_resolution, tile_size;
};
struct ImageProject { // project::Image, project/mod.rs:111-118
    uint32_t width = 0, height = 0;
    std::optional<Expression> filter, white;
};
struct Project {
    ImageProject image;
    CameraProject camera;
    RendererProject renderer;
    WorldProject world;
};

// ------------------------------------------------------------------------------------------------ the frozen scene
// What World::from_project + Resources hold, flattened into the arrays PyrSceneDesc points at.
class FlatScene {
  public:
    FlatScene();
    ~FlatScene();
    FlatScene(const FlatScene&) = delete;
    FlatScene& operator=(const FlatScene&) = delete;

    // ProgramCompiler::compile. Returns the program's index.
    uint32_t compile(const Expression& expression, bool allow_wavelength = true, bool vector_output = false);
    // Material::from_project: (material index, has emissive components)
    std::pair<uint32_t, bool> add_material(const Material& material);
    void add_world(const WorldProject& world, const std::string& base_dir = ".");
    void add_triangle(const float positions[9], const float normals[9], const float uvs[6], uint32_t material, const float frames[12] = nullptr);

    const PyrSceneDesc& desc(); // borrows this object's arrays
    // New places for the same primitives (World::update): [n][3][3] positions and normals, [n][3][4] frames, [n][4] spheres; an
    // empty vector leaves that array as it is, any other size than the scene's is a ProjectError
    void move_geometry(const std::vector<float>& positions, const std::vector<float>& normals, const std::vector<float>& frames, const std::vector<float>& spheres);
    size_t num_triangles() const;
    size_t num_spheres() const;
    size_t num_planes() const;
    // What moves together (World::pose): one record per project object that has geometry -- a sphere; a mesh -- in project order.
    struct Object {
        std::string name; // "objects[i]"
        PyrObjectRange range;
    };
    const std::vector<Object>& objects() const;

  private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// Corner labels for World::set_smoothing from a mesh's own arrays, [num_triangles][3][3] each: two corners get the same label
// exactly when the bits of their positions and of their normals agree in all six words, so a mesh keeps the creases its normals
// already have. A label is the index of the first corner of its group.
std::vector<uint32_t> weld(const float* positions, const float* normals, size_t num_triangles);

class World { // world.rs:31-36
  public:
    static std::unique_ptr<World> from_project(const WorldProject& world, const std::string& base_dir = ".");
    ~World();
    // Who builds the acceleration structure (pyr_scene_create_with): one host thread, or the device with the same rules and, where
    // no node needs the median fallback, the same tree. The builder is chosen when a scene is first used (none given: the host);
    // later calls get that scene, and naming another builder for it then is a ProjectError, as in the Python layer.
    enum class Build { Host, Device };
    PyrScene* scene(int device = 0, int copy = 0, std::optional<Build> build = std::nullopt); // created on first use (BVH build + upload); `copy` > 0: a further scene on the same device
    PyrBuildInfo build_info(int device = 0, int copy = 0); // pyr_scene_build_info: the builder used, why if not the one asked for, stage times, tree digest
    // Moves the geometry of the scene on `device` (pyr_scene_update, host arrays, blocking): new positions [n][3][3], normals
    // [n][3][3] and frames [n][3][4] for the same triangles, spheres [n][4] for the same spheres; an empty vector stays. Refit keeps
    // the tree's topology and recomputes every box on the device, Rebuild builds a new tree with the scene's builder. flat()
    // follows, so the description and the device agree.
    enum class Update { Refit, Rebuild };
    void update(const std::vector<float>& positions, const std::vector<float>& normals = {}, const std::vector<float>& frames = {},
                const std::vector<float>& spheres = {}, Update mode = Update::Refit, int device = 0);
    PyrUpdateInfo update_info(int device = 0); // pyr_scene_update_info: the last update's stages and the tree's area ratio
    // Poses the objects of the scene on `device` (pyr_scene_set_objects when the scene is made, pyr_scene_pose here): `poses` maps an
    // object's index in objects() to a column-major matrix (last row 0,0,0,1) and the uniform scale that comes first; objects it
    // does not name keep the identity -- every pose is from the rest pose, never from the previous one. The primitives are computed
    // on the GPU. flat() stays the rest pose; the world remembers the poses and a scene it makes later is built for them.
    struct ObjectPose {
        float transform[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        float scale = 1.0f;
    };
    const std::vector<FlatScene::Object>& objects() const { return flat_.objects(); }
    void pose(const std::map<size_t, ObjectPose>& poses, Update mode = Update::Refit, int device = 0, void* hip_stream = nullptr);
    // Names the description's objects again on every scene of this world (pyr_scene_set_objects): the geometry as it is now is the
    // rest pose, every pose the identity. An update() that carried arrays makes the scene forget its objects until this is called.
    void set_objects();
    // Binds meshes to joints (pyr_scene_set_skins on every scene of this world): `skins` maps an object's index in objects() to its
    // bindings -- four joint indices below num_joints and four weights for each of the three vertices of each of the object's
    // triangles ([T][3][4] each). Skins are in the order of their object indices. Every joint is the identity afterwards and the
    // geometry does not change; an empty map forgets the skins, and so do set_objects() and an update() that carries arrays.
    // `blend`: PYR_SKIN_LINEAR (the vertex's matrix is the weighted sum of its joints' matrices) or PYR_SKIN_DUAL_QUATERNION
    // (pyr_scene_set_skin_blend: the joints are blended as rigid motions, which keeps the volume of a twisting mesh; the joints of
    // such a skin must be rotations and translations).
    struct Skin {
        uint32_t num_joints = 0;
        std::vector<uint16_t> joints;
        std::vector<float> weights;
        uint32_t blend = PYR_SKIN_LINEAR;
    };
    void set_skins(const std::map<size_t, Skin>& skins);
    // One frame of the skinned meshes of the scene on `device` (pyr_scene_skin): `joints` maps a skinned object's index to its joint
    // matrices, 16 floats each, column-major with last row 0,0,0,1; a skin it does not name is at the identity. Every vertex takes
    // the matrix blended from its four joints by its weights, then the object's pose: `poses` as for pose(), nullptr keeps the
    // poses the world is in. Everything is computed from the rest pose on the GPU. flat() stays the rest pose; the world remembers
    // joints and poses and a scene it makes later is built for them.
    void skin(const std::map<size_t, std::vector<float>>& joints, const std::map<size_t, ObjectPose>* poses = nullptr, Update mode = Update::Refit, int device = 0,
              void* hip_stream = nullptr);
    // Gives meshes their morph targets (pyr_scene_set_morphs on every scene of this world): `morphs` maps an object's index in
    // objects() to its targets -- position deltas [num_targets][T][3][3] for the object's T triangles and, if the normals are to
    // follow, normal deltas of the same shape (empty: normals and frames stay the rest pose's). Morphs are in the order of their
    // object indices. Every weight is zero afterwards and the geometry does not change; an empty map forgets the morphs, and so do
    // set_objects() and an update() that carries arrays. set_skins() and set_morphs() leave each other's state alone.
    struct Morph {
        uint32_t num_targets = 0;
        std::vector<float> position_deltas, normal_deltas;
    };
    void set_morphs(const std::map<size_t, Morph>& morphs);
    // One frame of the morphed meshes of the scene on `device` (pyr_scene_morph): `weights` maps a morphed object's index to one
    // weight per target; a morph it does not name stays at the weights it is in. Every vertex takes the weighted deltas of the
    // targets whose weight is not zero, then its skin if its object has one (`joints` as for skin(), nullptr keeps the joints the
    // world is in), then the object's pose (`poses` as for pose(), nullptr keeps them). Everything is computed from the rest pose
    // on the GPU. flat() stays the rest pose; the world remembers weights, joints and poses for a scene it makes later.
    void morph(const std::map<size_t, std::vector<float>>& weights, const std::map<size_t, std::vector<float>>* joints = nullptr,
               const std::map<size_t, ObjectPose>* poses = nullptr, Update mode = Update::Refit, int device = 0, void* hip_stream = nullptr);
    // Has the normals of meshes recomputed from where their surface is (pyr_scene_set_smoothing on every scene of this world):
    // `smoothing` maps an object's index in objects() to one label per corner of the object's T triangles, [T][3] -- corners with
    // equal labels share a vertex normal, the area-weighted sum of their triangles' face vectors -- or to an empty vector: weld()
    // of the object's rest positions and rest normals. From then on every pose(), skin() and morph() recomputes those objects'
    // normals and tangent frames on the GPU from the frame's positions, also under the identity. The geometry does not change at
    // this call; an empty map forgets the smoothing, and so do set_objects() and an update() that carries arrays.
    void set_smoothing(const std::map<size_t, std::vector<uint32_t>>& smoothing);
    // pyr_scene_geometry: the geometry of the scene on `device` as it is now (frames empty unless the scene keeps them)
    struct Geometry {
        std::vector<float> positions, normals, frames, spheres;
    };
    Geometry geometry(int device = 0);
    // pyr_scene_keep_previous: keeps the geometry of the scene on `device` as it is now as the previous frame's, for
    // Renderer::motion; whatever update, pose or skin follows leaves it alone. `keep` false drops it.
    void keep_previous(bool keep = true, int device = 0);
    // World::intersect (world.rs:273-299) for a batch of rays, [n][6] = origin, direction: closest hits, on the GPU
    std::vector<PyrHit> intersect(const std::vector<float>& rays, int device = 0, PyrCounters* counters = nullptr);
    FlatScene& flat() { return flat_; }
    size_t num_objects() { return flat_.num_triangles() + flat_.num_spheres() + flat_.num_planes(); } // world.rs:251-254

  private:
    World() = default;
    FlatScene flat_;
    std::map<std::pair<int, int>, PyrScene*> scenes_;
    std::map<std::pair<int, int>, Build> builders_; // what each scene was asked to be built by
    std::map<size_t, ObjectPose> poses_;            // the poses the scenes are in; identity where absent
    std::map<size_t, Skin> skins_;                  // the bindings (set_skins)
    std::map<size_t, std::vector<float>> joints_;   // the joints the scenes are in; identity where absent
    std::map<size_t, Morph> morphs_;                // the targets (set_morphs)
    std::map<size_t, std::vector<float>> weights_;  // the morph weights the scenes are in; zero where absent
    std::map<size_t, std::vector<uint32_t>> smoothing_; // the corner labels (set_smoothing)
    bool smooth_frame_ = false;                     // a pose, skin or morph has run since: the scenes hold recomputed normals
    std::vector<PyrObjectPose> pose_records(const std::map<size_t, ObjectPose>& poses) const;
    void set_skins_on(PyrScene* handle, const std::map<size_t, Skin>& skins);
    std::vector<float> joint_table(const std::map<size_t, std::vector<float>>& joints) const;
    void set_morphs_on(PyrScene* handle, const std::map<size_t, Morph>& morphs);
    void set_smoothing_on(PyrScene* handle, const std::map<size_t, std::vector<uint32_t>>& smoothing);
    // pose, skin and morph are one frame: `entry` says which of pyr_scene_pose, pyr_scene_skin and pyr_scene_morph runs and names the
    // errors; a table the entry has not, or a nullptr, keeps what the world is in. send_frame fills the widest update the entry has.
    enum class Entry { Pose, Skin, Morph };
    using Tables = std::map<size_t, std::vector<float>>;
    void frame(Entry entry, const Tables* weights, const Tables* joints, const std::map<size_t, ObjectPose>* poses, Update mode, int device, void* hip_stream);
    void send_frame(PyrScene* handle, Entry entry, const Tables& weights, const Tables* joints, const std::map<size_t, ObjectPose>& poses, Update mode, void* hip_stream);
    void forget(); // every pose is the identity again, and what hangs on objects is gone
};

struct Camera { // cameras.rs:20-27
    PyrCamera c{};
    static Camera from_project(const CameraProject& camera);
};

class Film { // film.rs:9-18
  public:
    Film(uint32_t width, uint32_t height, uint32_t grains_per_pixel = 64, float wavelength_start = 380.0f, float wavelength_end = 780.0f);
    PyrFilmDesc desc() const;
    uint32_t width, height, bins;
    float wavelength_start, wavelength_width;
    std::vector<PyrGrain> grains; // (x + y * width) * bins + bin, film.rs:56
    double total_weight() const;
    // main.rs:315-327: develop into 8-bit sRGB [height][width][3] on the GPU, with the image's filter / white programs.
    std::vector<uint8_t> develop(const std::optional<Expression>& filter = std::nullopt, const std::optional<Expression>& white = std::nullopt,
                                 float step_size = 2.0f, int device = 0) const;
};
void save_png(const std::string& path, const std::vector<uint8_t>& rgb, uint32_t width, uint32_t height);

// ---- linear images and tone mapping (pyrite_gpu.h "linear images and tone mapping"; pyrite_amd/develop.py has the same surface) ----
// [height][width][3] f32 of `film` (+ `film_b`, grain by grain) on the GPU: CIE XYZ or the linear sRGB triple Film::develop clamps and encodes.
std::vector<float> develop_linear(const Film& film, uint32_t space = PYR_LINEAR_SRGB, const std::optional<Expression>& filter = std::nullopt,
                                  const std::optional<Expression>& white = std::nullopt, float step_size = 2.0f, int device = 0, const Film* film_b = nullptr);
PyrImageStats image_stats(const std::vector<float>& linear_srgb, uint32_t width, uint32_t height, int device = 0);
// exposure / white <= 0: automatic (pyr_tone_resolve)
PyrToneParams tone_params(uint32_t op = PYR_TONE_CLIP, float exposure = 0.0f, float white = 0.0f);
// 8-bit sRGB of a linear sRGB image; what `tone` leaves automatic is resolved from the image's statistics, taken here.
std::vector<uint8_t> tonemap(const std::vector<float>& linear_srgb, uint32_t width, uint32_t height, const PyrToneParams& tone, int device = 0);
// The bytes of a Radiance RGBE picture (flat scanlines) and of a colour PFM file (little-endian, rows bottom to top) of a linear
// image, pure functions (csrc/host/images.cpp; pyrite_amd/develop.py encode_hdr / encode_pfm write the same bytes). RGBE is Ward's
// mapping in f64: a channel that is not positive is 0, one above kRgbeMax (+inf too) is kRgbeMax; m = the largest channel;
// m < 1e-32: four zero bytes; else m = f * 2^e, f in [0.5, 1): mantissa bytes (uint8)(c * (f * 256 / m)), exponent byte e + 128.
constexpr double kRgbeMax = 255.0 * 0x1p119; // the largest value a pixel holds: mantissa 255, exponent byte 255
std::vector<uint8_t> encode_hdr(const std::vector<float>& rgb, uint32_t width, uint32_t height);
std::vector<uint8_t> encode_pfm(const std::vector<float>& rgb, uint32_t width, uint32_t height);
void write_hdr(const std::string& path, const std::vector<float>& rgb, uint32_t width, uint32_t height);
void write_pfm(const std::string& path, const std::vector<float>& rgb, uint32_t width, uint32_t height);
void write_linear(const std::string& path, const std::vector<float>& rgb, uint32_t width, uint32_t height); // --hdr PATH: .hdr or .pfm by the extension
// What is wrong with --hdr / --exposure / --tone, in the words both front ends print, or "" (pyrite_amd/develop.py tone_flag_problem).
std::string tone_flag_problem(const std::optional<std::string>& hdr, const std::optional<std::string>& exposure, const std::optional<std::string>& tone);
// The tone parameters of --exposure EV|auto and --tone clip|reinhard, or nothing when neither is given (pyrite_amd/develop.py tone_from_flags).
std::optional<PyrToneParams> tone_from_flags(const std::optional<std::string>& exposure, const std::optional<std::string>& tone);

// ---- denoising (pyrite_gpu.h "denoising a linear image from two halves"; pyrite_amd/develop.py denoise has the same surface) ----
// The defaults: PYR_DENOISE_RADIUS, PYR_DENOISE_PATCH, PYR_DENOISE_K, PYR_DENOISE_EPSILON and the three guide sigmas.
PyrDenoiseParams denoise_params(uint32_t radius = PYR_DENOISE_RADIUS, uint32_t patch = PYR_DENOISE_PATCH);
// What denoise and Session::denoised return: the filtered image and the noise that is left, [height][width][3] f32 each.
struct Denoised {
    std::vector<float> image, error;
};
// The two half images `a` and `b` (linear light, independent samples of one picture) cross filtered on the GPU (pyr_image_denoise).
// Guides, either may be null: `albedo`, a linear image, and `pixels`, the records of the feature pass.
Denoised denoise(const std::vector<float>& a, const std::vector<float>& b, uint32_t width, uint32_t height, const PyrDenoiseParams& params = denoise_params(),
                 const std::vector<float>* albedo = nullptr, const std::vector<PyrFeaturePixel>* pixels = nullptr, int device = 0);
// What is wrong with --denoise / --denoise-radius, in the words both front ends print, or "" (pyrite_amd/develop.py
// denoise_flag_problem). `pixel_samples`: the render's budget once the project is loaded; `pass_samples`: --pass-samples, when given.
std::string denoise_flag_problem(bool denoise, const std::optional<long>& denoise_radius, const std::optional<uint32_t>& pixel_samples = std::nullopt,
                                 const std::optional<long>& pass_samples = std::nullopt);

// ---- accumulation over frames (pyrite_gpu.h "motion records and accumulation over frames"; pyrite_amd/develop.py reproject) ----
// What reproject returns: the running mean, [height][width][3] f32, and the frames each pixel's mean holds, [height][width] f32.
struct Accumulated {
    std::vector<float> image, count;
};
PyrReprojectParams reproject_params(float depth_tolerance = PYR_REPROJECT_DEPTH_TOLERANCE, float max_history = PYR_REPROJECT_MAX_HISTORY);
// `current` with the records of its frame (Renderer::motion), accumulated onto `history` -- the previous call's result and the
// records of that frame; both null for a first frame (pyr_image_reproject).
Accumulated reproject(const std::vector<float>& current, const std::vector<PyrMotionPixel>& motion, uint32_t width, uint32_t height, const Accumulated* history = nullptr,
                      const std::vector<PyrMotionPixel>* history_motion = nullptr, const PyrReprojectParams& params = reproject_params(), int device = 0);

// ---- temporal resolve (pyrite_gpu.h "temporal resolve"; pyrite_amd/develop.py resolve) ----
// What resolve returns: reproject's image and count, and how far outside the clip box each pixel's history lay, [height][width] f32.
struct Resolved {
    std::vector<float> image, count, clip;
};
PyrTemporalParams temporal_params(float depth_tolerance = PYR_REPROJECT_DEPTH_TOLERANCE, float max_history = PYR_REPROJECT_MAX_HISTORY, uint32_t radius = PYR_TEMPORAL_RADIUS,
                                  float gamma = PYR_TEMPORAL_GAMMA, float noise_scale = PYR_TEMPORAL_NOISE_SCALE, float response = PYR_TEMPORAL_RESPONSE);
// reproject with the fetched history clipped to the neighbourhood of `current` (pyr_image_temporal_resolve). `history`: the image and
// count of the previous call's result (a Resolved's image and count in an Accumulated), with the records of that frame; both null for a
// first frame. `noise`: the error image of the denoiser for this frame, or null. A buffer of another size than the image's is a
// ProjectError before the library is called.
Resolved resolve(const std::vector<float>& current, const std::vector<PyrMotionPixel>& motion, uint32_t width, uint32_t height, const Accumulated* history = nullptr,
                 const std::vector<PyrMotionPixel>* history_motion = nullptr, const std::vector<float>* noise = nullptr, const PyrTemporalParams& params = temporal_params(),
                 int device = 0);

// ---- motion blur over the motion records (pyrite_gpu.h "motion blur over the motion records"; pyrite_amd/develop.py motion_blur) ----
PyrMotionBlurParams motion_blur_params(float shutter = PYR_MOTION_BLUR_SHUTTER, uint32_t samples = PYR_MOTION_BLUR_SAMPLES, uint32_t max_radius = PYR_MOTION_BLUR_MAX_RADIUS,
                                       float depth_softness = PYR_MOTION_BLUR_DEPTH_SOFTNESS, uint32_t seed = 0);
// The linear image `image`, [height][width][3] f32, blurred along the records of its frame (Renderer::motion) on the GPU
// (pyr_image_motion_blur). A buffer of another size than the image's is a ProjectError before the library is called.
std::vector<float> motion_blur(const std::vector<float>& image, const std::vector<PyrMotionPixel>& motion, uint32_t width, uint32_t height,
                               const PyrMotionBlurParams& params = motion_blur_params(), int device = 0);

// ---- lens blur over the feature records (pyrite_gpu.h "lens blur over the feature records"; pyrite_amd/develop.py lens_blur) ----
PyrLensBlurParams lens_blur_params(float focus_distance, float aperture, float view_plane, uint32_t max_radius = PYR_LENS_BLUR_MAX_RADIUS,
                                   float depth_tolerance = PYR_REPROJECT_DEPTH_TOLERANCE);
// The three lens numbers of `camera`.
PyrLensBlurParams lens_blur_params(const Camera& camera, uint32_t max_radius = PYR_LENS_BLUR_MAX_RADIUS, float depth_tolerance = PYR_REPROJECT_DEPTH_TOLERANCE);
// The linear image `image`, [height][width][3] f32, rendered through a pinhole, blurred as a thin lens would blur it, over the
// feature records of the same camera at the same size (Renderer::features) on the GPU (pyr_image_lens_blur). A buffer of another
// size than the image's is a ProjectError before the library is called.
std::vector<float> lens_blur(const std::vector<float>& image, const std::vector<PyrFeaturePixel>& pixels, uint32_t width, uint32_t height, const PyrLensBlurParams& params,
                             int device = 0);
// What is wrong with --lens-blur / --lens-blur-radius R, in the words both front ends print, or "" (pyrite_amd/develop.py lens_blur_flag_problem).
std::string lens_blur_flag_problem(bool lens_blur, const std::optional<long>& lens_blur_radius);

// ---- glare (pyrite_gpu.h "glare"; pyrite_amd/develop.py glare) ----
PyrGlareParams glare_params(float strength = PYR_GLARE_STRENGTH, uint32_t levels = PYR_GLARE_LEVELS, float threshold = PYR_GLARE_THRESHOLD, float falloff = PYR_GLARE_FALLOFF);
// The linear image `image`, [height][width][3] f32, with the glare of a lens or an eye added on the GPU (pyr_image_glare). A buffer
// of another size than the image's is a ProjectError before the library is called.
std::vector<float> glare(const std::vector<float>& image, uint32_t width, uint32_t height, const PyrGlareParams& params = glare_params(), int device = 0);
// What is wrong with --glare / --glare-levels / --glare-threshold, in the words both front ends print, or "" (pyrite_amd/develop.py
// glare_flag_problem). `glare`: the strength as it was given, or nothing without --glare.
std::string glare_flag_problem(const std::optional<std::string>& glare, const std::optional<long>& glare_levels, const std::optional<double>& glare_threshold);
// The parameters of --glare [STRENGTH] --glare-levels N --glare-threshold T, or nothing without --glare (pyrite_amd/develop.py glare_from_flags).
std::optional<PyrGlareParams> glare_from_flags(const std::optional<std::string>& glare, const std::optional<long>& glare_levels, const std::optional<double>& glare_threshold);

// ---- guided upsampling (pyrite_gpu.h "upsample"; pyrite_amd/develop.py upsample) ----
PyrUpsampleParams upsample_params(uint32_t radius = PYR_UPSAMPLE_RADIUS, bool match_material = true, float sigma_normal = PYR_UPSAMPLE_SIGMA_NORMAL,
                                  float sigma_depth = PYR_UPSAMPLE_SIGMA_DEPTH, float albedo_floor = PYR_UPSAMPLE_ALBEDO_FLOOR, float max_gain = PYR_UPSAMPLE_MAX_GAIN);
// The linear image `low`, [low_height][low_width][3] f32, upsampled `scale` times on the GPU (pyr_image_upsample). The albedo pair
// (`low_albedo` of low's size, `albedo` of the result's) and the records pair (`low_pixels`, `pixels`) are each given whole or not at
// all. A buffer of another size than its image's, or half a pair, is a ProjectError before the library is called.
std::vector<float> upsample(const std::vector<float>& low, uint32_t low_width, uint32_t low_height, uint32_t scale, const PyrUpsampleParams& params = upsample_params(),
                            const std::vector<float>* albedo = nullptr, const std::vector<PyrFeaturePixel>* pixels = nullptr, const std::vector<float>* low_albedo = nullptr,
                            const std::vector<PyrFeaturePixel>* low_pixels = nullptr, int device = 0);
// What is wrong with --upsample N / --upsample-radius R, in the words both front ends print, or "" (pyrite_amd/develop.py
// upsample_flag_problem). `width`, `height`: the image's size once the project is loaded -- N must divide both.
std::string upsample_flag_problem(const std::optional<long>& upsample, const std::optional<long>& upsample_radius, const std::optional<uint32_t>& width = std::nullopt,
                                  const std::optional<uint32_t>& height = std::nullopt);
// The parameters of --upsample N --upsample-radius R, or nothing without --upsample (pyrite_amd/develop.py upsample_from_flags).
std::optional<PyrUpsampleParams> upsample_from_flags(const std::optional<long>& upsample, const std::optional<long>& upsample_radius);

// ---- despeckle (pyrite_gpu.h "despeckle"; pyrite_amd/develop.py despeckle) ----
PyrDespeckleParams despeckle_params(uint32_t radius = PYR_DESPECKLE_RADIUS, float k = PYR_DESPECKLE_K, float relative = PYR_DESPECKLE_RELATIVE, float floor = PYR_DESPECKLE_FLOOR);
// What despeckle returns: the cleaned halves (b empty when none was given), what the mean of the halves lost, [height][width][3]
// f32 each, and the pixels clamped in a and in b.
struct Despeckled {
    std::vector<float> a, b, removed;
    uint32_t counts[2];
};
// The half images `a` and `b` (linear light, independent samples of one picture; `b` may be null: one image, no agreement test)
// with their fireflies clamped on the GPU (pyr_image_despeckle). A buffer of another size than the image's is a ProjectError
// before the library is called.
Despeckled despeckle(const std::vector<float>& a, const std::vector<float>* b, uint32_t width, uint32_t height, const PyrDespeckleParams& params = despeckle_params(),
                     int device = 0);
// What is wrong with --despeckle [K] / --despeckle-radius R, in the words both front ends print, or "" (pyrite_amd/develop.py
// despeckle_flag_problem). `despeckle`: K as it was given, or nothing without --despeckle.
std::string despeckle_flag_problem(const std::optional<std::string>& despeckle, const std::optional<long>& despeckle_radius,
                                   const std::optional<uint32_t>& pixel_samples = std::nullopt, const std::optional<long>& pass_samples = std::nullopt);
// The parameters of --despeckle [K] --despeckle-radius R, or nothing without --despeckle (pyrite_amd/develop.py despeckle_from_flags).
std::optional<PyrDespeckleParams> despeckle_from_flags(const std::optional<std::string>& despeckle, const std::optional<long>& despeckle_radius);
// What Session::despeckled returns: the image, the noise left, what the clamp removed and the pixels clamped in either half.
struct DespeckledImage {
    std::vector<float> image, error, removed;
    uint32_t counts[2];
};

struct Progress { // renderer/mod.rs:229-232
    uint8_t progress;
    const char* message;
};

class Renderer { // renderer/mod.rs:18-28, Algorithm::Simple
  public:
    uint32_t bounces = 8, pixel_samples = 1, light_samples = 4, spectrum_samples = 10, spectrum_bins = 64, tile_size = 32;
    float spectrum_span[2] = {380.0f, 780.0f};
    uint64_t seed = 1; // no reference counterpart: the reference seeds from OS entropy (simple.rs:26-28)
    static Renderer from_project(const RendererProject& renderer);
    Film new_film(uint32_t width, uint32_t height) const { return Film(width, height, spectrum_bins, spectrum_span[0], spectrum_span[1]); } // main.rs:190-195
    // The seam: blocking; adds into `film`; `on_status` runs on the calling thread. Returns the kernel counters when asked to.
    void render(Film& film, const Camera& camera, World& world, const std::function<void(Progress)>& on_status = nullptr, int device = 0,
                PyrCounters* counters = nullptr) const;
    // The same seam over several GPUs of this process (pyr_render_simple_multi): the scene is replicated on every listed
    // device, the image's tiles are dealt round-robin, one launch per device, one RCCL gather of the film blocks to
    // devices[0]. What the reference does with its worker threads (renderer/mod.rs:125-189) a host does with its GPUs.
    // A device listed twice is the one-GPU test rig (pyrite_gpu.h).
    void render(Film& film, const Camera& camera, World& world, const std::vector<int>& devices, const std::function<void(Progress)>& on_status = nullptr) const;
    PyrRenderParams params(uint32_t sample_begin = 0) const; // this renderer as the ABI's parameter block
    // The first-hit feature images (pyr_render_features; pyrite_amd/renderer.py Renderer.features): no noise, no random numbers.
    struct Features features(uint32_t width, uint32_t height, const Camera& camera, World& world, uint32_t grid = 1, uint32_t albedo_bins = 16, int device = 0) const;
    // The motion records (pyr_render_motion; pyrite_amd/renderer.py Renderer.motion), one per pixel, row-major: where the surface
    // point `camera` sees was for `previous_camera` in the geometry World::keep_previous kept (none kept: the geometry as it is).
    std::vector<PyrMotionPixel> motion(uint32_t width, uint32_t height, const Camera& camera, World& world, const Camera& previous_camera, int device = 0) const;
};

// What Renderer::features and Session::features return: the albedo film (albedo_bins bins over the renderer's span; develop and
// save_png apply) and one PyrFeaturePixel per pixel, row-major (pyrite_gpu.h "first-hit feature images").
struct Features {
    Film albedo;
    std::vector<PyrFeaturePixel> pixels;
};
// The 8-bit images of the records, [height][width][3], pure functions (pyrite_amd/features.py encode_normal / encode_depth write
// the same bytes): normal = (uint8)(255 * (0.5 * n + 0.5) + 0.5) per channel in f32; depth = grey, linear between the smallest and
// the largest depth over the pixels with coverage > 0, near is white. Pixels with coverage 0 are black in both.
std::vector<uint8_t> encode_normal_image(const std::vector<PyrFeaturePixel>& pixels);
std::vector<uint8_t> encode_depth_image(const std::vector<PyrFeaturePixel>& pixels);
// PREFIX_albedo.png (developed with the image's filter / white programs, step 2), PREFIX_normal.png, PREFIX_depth.png
void write_feature_images(const std::string& prefix, const Features& features, const std::optional<Expression>& filter = std::nullopt,
                          const std::optional<Expression>& white = std::nullopt, int device = 0);
// What is wrong with --features / --features-grid, in the words both front ends print, or "" (pyrite_amd/features.py features_flag_problem).
std::string features_flag_problem(bool features, const std::optional<long>& features_grid);

// A render cut into passes over the whole image (pyrite_gpu.h "progressive sessions"): the film lives on the GPU, render()
// enqueues the next samples of every pixel and returns at once, preview() develops the live film there and fetches the 8-bit image
// alone. The world's scene on that device serves this session alone while it renders. pyrite_amd/renderer.py Session is the same.
class Session {
  public:
    Session(const Renderer& renderer, uint32_t width, uint32_t height, const Camera& camera, World& world, bool halves = false, int device = 0,
            const Film* start = nullptr);
    ~Session();
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    void render(uint32_t samples);
    void sync();
    uint32_t samples_done() const;
    // main.rs:261-299: [height][width][3] sRGB of the film as it stands, with the image's filter / white programs
    std::vector<uint8_t> preview(float step_size = 30.0f, const std::optional<Expression>& filter = std::nullopt, const std::optional<Expression>& white = std::nullopt);
    // pyr_session_preview_tone: the preview through a tone curve; `stats`, when given, receives the linear image's statistics
    std::vector<uint8_t> preview_tone(const PyrToneParams& tone, float step_size = 30.0f, const std::optional<Expression>& filter = std::nullopt,
                                      const std::optional<Expression>& white = std::nullopt, PyrImageStats* stats = nullptr);
    // pyr_session_linear: [height][width][3] f32, the film as it stands in linear light
    std::vector<float> linear(uint32_t space = PYR_LINEAR_SRGB, float step_size = 2.0f, const std::optional<Expression>& filter = std::nullopt,
                              const std::optional<Expression>& white = std::nullopt);
    Film film();
    std::vector<float> noise(); // per tile of the make_tiles grid, raster order (pyr_session_noise): needs halves and two passes
    Features features(uint32_t grid = 1, uint32_t albedo_bins = 16); // pyr_session_features: after the passes enqueued so far; the film is not touched
    std::vector<PyrMotionPixel> motion(const Camera& previous_camera); // pyr_session_motion: the session's camera against the previous one; the film is not touched
    // pyr_session_motion_blurred: the film as it stands in linear sRGB, blurred along the records against `previous_camera`, on the session's device
    std::vector<float> motion_blurred(const Camera& previous_camera, const PyrMotionBlurParams& params = motion_blur_params(), float step_size = 2.0f,
                                      const std::optional<Expression>& filter = std::nullopt, const std::optional<Expression>& white = std::nullopt);
    // pyr_session_lens_blurred: the film as it stands in linear sRGB, blurred by the lens of `params` over the records of the feature
    // pass (grid x grid sub-samples), on the session's device; the film is not touched
    std::vector<float> lens_blurred(const PyrLensBlurParams& params, uint32_t grid = 1, float step_size = 2.0f, const std::optional<Expression>& filter = std::nullopt,
                                    const std::optional<Expression>& white = std::nullopt);
    // pyr_session_glared: the film as it stands in linear sRGB with the glare added, on the session's device; the film is not touched
    std::vector<float> glared(const PyrGlareParams& params = glare_params(), float step_size = 2.0f, const std::optional<Expression>& filter = std::nullopt,
                              const std::optional<Expression>& white = std::nullopt);
    // pyr_session_denoised: the two half films developed to linear sRGB and cross filtered on the session's device; with `guides` the
    // feature pass (grid, albedo_bins) runs first and steers the filter. Needs halves and two passes; the films are not touched.
    Denoised denoised(const PyrDenoiseParams& params = denoise_params(), bool guides = true, float step_size = 2.0f, const std::optional<Expression>& filter = std::nullopt,
                      const std::optional<Expression>& white = std::nullopt, uint32_t grid = 1, uint32_t albedo_bins = 16);
    // pyr_session_upsampled: the film, the low image, in linear sRGB -- with `denoise` what denoised() gives -- upsampled `scale`
    // times under the guidance of the feature pass (grid, albedo_bins) at both sizes, on the session's device: [scale*height]
    // [scale*width][3] f32. Without `guides` no feature pass runs: the plain tent. The films are not touched.
    std::vector<float> upsampled(uint32_t scale, const PyrUpsampleParams& params = upsample_params(), bool guides = true, const std::optional<PyrDenoiseParams>& denoise = std::nullopt,
                                 float step_size = 2.0f, const std::optional<Expression>& filter = std::nullopt, const std::optional<Expression>& white = std::nullopt,
                                 uint32_t grid = 1, uint32_t albedo_bins = 16);
    // pyr_session_despeckled: the two half films developed to linear sRGB, their fireflies clamped, then cross filtered as denoised()
    // filters the raw halves (`denoise`; `guides`, grid, albedo_bins: its feature pass) or, without `denoise`, their mean and half
    // their difference, on the session's device. Needs halves and two passes; the films are not touched.
    DespeckledImage despeckled(const PyrDespeckleParams& params = despeckle_params(), const std::optional<PyrDenoiseParams>& denoise = std::nullopt, bool guides = true,
                               float step_size = 2.0f, const std::optional<Expression>& filter = std::nullopt, const std::optional<Expression>& white = std::nullopt,
                               uint32_t grid = 1, uint32_t albedo_bins = 16);
    uint32_t tiles_x() const { return (width_ + tile_size_ - 1) / tile_size_; }
    uint32_t tiles_y() const { return (height_ + tile_size_ - 1) / tile_size_; }

  private:
    PyrSession* handle_ = nullptr;
    Film shape_; // the film's description (no grains are kept here)
    uint32_t width_, height_, tile_size_;
};

// What is wrong with the flags of a progressive render (--pass-samples, --preview-every, --noise without --preview), in the words
// both front ends print, or "" (pyrite_amd/__main__.py progressive_flag_problem).
std::string progressive_flag_problem(const std::optional<long>& pass_samples, bool preview, double preview_every, bool noise);
constexpr uint32_t kDefaultPassSamples = 256; // passes of a render with a preview when --pass-samples is not given: the smallest that cost nothing on C3

// ------------------------------------------------------------------------------------------------ project files
// Reads a project file (*.lua): the declarative subset of Lua project files are written in, evaluated against the prelude
// of pyrite/src/project/lib.lua, then typed_nodes' FromLua step (pyrite_amd/csrc/host/lua_project.cpp; main.rs:111-134).
// Image files are decoded by `textures`, which turns (absolute path, linear?, mono?) into linear f32 texels
// ([height][width][4] or [height][width]) -- what Texture::from_path does (texture.rs:25-85). One texture per (file, kind).
using TextureLoader = std::function<std::vector<float>(const std::string& path, bool linear, bool mono, uint32_t& width, uint32_t& height)>;
struct LoadedProject {
    Project project;
    std::string base_dir; // mesh and texture paths are relative to the project file's directory (project/mod.rs:73-76)
};
// The built-in decoder: PNG and baseline JPEG files -> linear texels (pyrite_amd/csrc/host/images.cpp). It is what
// load_project / evaluate_project use when no loader is given.
std::vector<float> load_texture_file(const std::string& path, bool linear, bool mono, uint32_t& width, uint32_t& height);
LoadedProject load_project(const std::string& path, const TextureLoader& textures = nullptr);
LoadedProject evaluate_project(const std::string& text, const std::string& name, const std::string& base_dir, const TextureLoader& textures = nullptr);

// Value of a wavelength-only expression with the VM's f32 arithmetic (image.filter / image.white, main.rs:470-518).
float evaluate_at(const Expression& expression, float wavelength);

} // namespace pyrite

// Canonical byte image of a PyrSceneDesc (every array with its length, in declaration order): equal scenes give equal
// bytes. Test infrastructure for comparing front-ends; returns the size needed, writes at most `capacity` bytes.
extern "C" uint64_t pyrh_serialize_desc(const PyrSceneDesc* desc, uint8_t* out, uint64_t capacity);
// pyrite::save_png through a C entry point (tests). Returns 0 on success.
extern "C" int64_t pyrh_test_load_texture(const char* path, int linear, int mono, float* out, uint64_t capacity, uint32_t* width, uint32_t* height);
extern "C" int pyrh_test_png(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height);
// pyrite::write_hdr (pfm == 0) / write_pfm through a C entry point (tests). Returns 0 on success.
extern "C" int pyrh_test_linear_image(const char* path, const float* rgb, uint32_t width, uint32_t height, int pfm);

#endif // PYRITE_HOST_HPP
