/*
 * pyrite_gpu.h -- C ABI of the MI355X-native replacement for Pyrite's camera-to-light
 * ("simple") renderer hot path.
 *
 * The reference (Ogeon/pyrite) has no FFI; the seam this ABI drops in behind is
 *
 *     Renderer::render(&self, film, task_runner, on_status, camera, world, resources)
 *         pyrite/src/renderer/mod.rs:77-111   (match Algorithm::Simple => simple::render, :87-89)
 *
 * i.e. everything the reference does from `simple::render` (pyrite/src/renderer/simple.rs:17-56)
 * downwards. A Rust caller binds these symbols with an `extern "C"` block
 * and calls them from a new `Algorithm::Gpu` arm.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++ / torch / HIP types in any signature
 *     (`hip_stream` is an opaque `void*` holding a hipStream_t, NULL = default stream);
 *   - the caller owns every input array and the film buffer; the library copies what it needs in
 *     pyr_scene_create and owns the returned PyrScene;
 *   - every function returns PYR_OK (0) or a negative PyrStatus and never aborts the process
 *     (the reference panics with panic=abort: Cargo.toml:6,10); pyr_last_error() returns a
 *     thread-local message for the last failure;
 *   - all floating point data is IEEE binary32, matrices are column-major (cgmath::Matrix4);
 *   - progress callbacks are only ever invoked on the calling thread
 *     (FnMut, not Send: pyrite/src/renderer/mod.rs:181-183).
 */
#ifndef PYRITE_GPU_H
#define PYRITE_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYR_ABI_VERSION 5

typedef enum PyrStatus {
    PYR_OK = 0,
    PYR_ERR_INVALID_ARGUMENT = -1,
    PYR_ERR_UNSUPPORTED = -2, /* outside what the library renders: ray-marched shapes (SURVEY.md section 8 "out" rows), a program beyond the
                                 wide register file, sizes beyond the bounds stated at pyr_scene_create */
    PYR_ERR_DEVICE = -3,      /* a HIP call failed or no gfx950 device is present */
    PYR_ERR_OUT_OF_MEMORY = -4
} PyrStatus;

/* ---------------------------------------------------------------- film ------------------------ */

/* == GrainData {accumulator, weight}: pyrite/src/film.rs:165-169 (field order acc, weight). */
typedef struct PyrGrain {
    float acc;
    float weight;
} PyrGrain;

/* == Film {width, height, grains_per_pixel, wavelength_start, wavelength_width}: film.rs:9-18.
 * Grain index = (x + y*width)*bins + bin  (film.rs:56). */
typedef struct PyrFilmDesc {
    uint32_t width;
    uint32_t height;
    uint32_t bins;
    float wl_start; /* 380 by default: renderer/mod.rs:16 */
    float wl_width; /* 400 by default */
} PyrFilmDesc;

/* ---------------------------------------------------------------- renderer parameters --------- */

#define PYR_FLAG_COUNTERS 1u /* run the instrumented kernel build and fill PyrCounters */

/* == Renderer {bounces, pixel_samples, light_samples, spectrum_samples, tile_size}
 * (renderer/mod.rs:18-28; defaults :63-75: 8 / - / 4 / 10 / 32). `threads` has no meaning here.
 *
 * The reference seeds one entropy RNG per tile (simple.rs:26-28) and is not reproducible; here
 * every sample (tile, iteration) owns a xorshift128 stream seeded from (seed, tile, iteration), see
 * DESIGN.md "RNG". `seed` selects the run.
 *
 * Sharding: a call renders the raster-order tile range [tile_begin, tile_end) (tile index
 * ty*tiles_x + tx over the grid of make_tiles, renderer/algorithm.rs:152-188); tile_end == 0 means
 * "all tiles"; with tile_stride > 1 only the tiles tile_begin, tile_begin + tile_stride, ... below tile_end are
 * rendered (the multi-GPU plan deals tiles round-robin: rank r of n renders tile_begin = r, tile_stride = n).
 * Tiles are independent units in the reference too: each has its own RNG and writes its own pixels
 * (renderer/simple.rs:36-55).
 *
 * Sample windows (ABI 5): a tile of w x h pixels (clipped to the image) runs w*h*pixel_samples iterations of the simple.rs:78 loop;
 * with sample_begin = b the call runs the iterations [w*h*b, w*h*(b + pixel_samples)) of every tile instead of the first
 * w*h*pixel_samples. The RNG key stays (seed, tile, iteration), so the windows [0,n), [n,2n), ... of k calls are together exactly the
 * samples of one call with k*n samples per pixel: added into one film they give that call's film up to the order of the float
 * additions. sample_begin = 0 is a plain render. A window whose end a single call could not reach (2^32 chunks) is PYR_ERR_UNSUPPORTED.
 *
 * film_layout says what the film buffer handed to the call holds:
 *   PYR_FILM_ROWS         pixel rows [film_row_begin, film_row_begin + film_row_count) of the image in the film.rs:56 layout
 *                         (film_row_count == 0 means the whole image);
 *   PYR_FILM_TILE_BLOCKS  one block per rendered tile, in the order the tiles are rendered: block k belongs to tile
 *                         tile_begin + k*stride and holds (tile_size + 2)^2 pixels x bins grains -- the tile's
 *                         tile_size x tile_size pixel square with a one-pixel ring around it; image pixel (x, y) sits
 *                         at block-local (x - tile_x0 + 1, y - tile_y0 + 1), row-major, bins grains per pixel. The ring is
 *                         there because Film::expose recomputes the pixel from the view-plane position (film.rs:233-246) and
 *                         rounding can move a sample drawn on a tile edge into the neighbouring pixel (~1e-6 per sample).
 *                         pyr_film_blocks_assemble[_device] adds such blocks into a whole-image film.
 * Exposures that map outside the buffer are dropped exactly like exposures outside the image (film.rs:51-54,92). */
#define PYR_FILM_ROWS 0u
#define PYR_FILM_TILE_BLOCKS 1u
typedef struct PyrRenderParams {
    uint32_t bounces;
    uint32_t pixel_samples;
    uint32_t light_samples;
    uint32_t spectrum_samples;
    uint32_t tile_size;
    uint32_t flags;
    uint64_t seed;
    uint32_t tile_begin;
    uint32_t tile_end;
    uint32_t film_row_begin;
    uint32_t film_row_count;
    uint32_t tile_stride; /* 0 and 1 both mean every tile of the range */
    uint32_t film_layout; /* PYR_FILM_ROWS | PYR_FILM_TILE_BLOCKS */
    uint32_t sample_begin; /* ABI 5: the call renders samples [sample_begin, sample_begin + pixel_samples) of every pixel's budget */
} PyrRenderParams;

/* == Camera::Perspective {transform, view_plane, focus_distance, aperture}: cameras.rs:20-27.
 * cam_to_world = look_at(from,to,up)^-1 (project/mod.rs:257-266), column-major.
 * view_plane = cos(fov/2)/sin(fov/2), fov in degrees (cameras.rs:43-45). */
typedef struct PyrCamera {
    float cam_to_world[16];
    float view_plane;
    float focus_distance;
    float aperture;
} PyrCamera;

/* ---------------------------------------------------------------- programs (the expression VM) */

/* Flattened form of Instruction / InstructionType (program/instruction.rs:12-119). */
typedef enum PyrOp {
    PYR_OP_NUMBER = 0,        /* NumberValue     {number=x.constant, output}                 :20-23 */
    PYR_OP_VECTOR = 1,        /* VectorValue     {x,y,z,w, output}                           :24-30 */
    PYR_OP_RGB = 2,           /* RgbValue        {red=x, green=y, blue=z, output}            :31-36 */
    PYR_OP_SPECTRUM = 3,      /* SpectrumValue   {wavelength=x, spectrum=a, output}          :37-41 */
    PYR_OP_COLOR_TEXTURE = 4, /* ColorTextureValue {texture_coordinates=b (vector input), texture=a, output (rgb)} :42-46 */
    PYR_OP_MONO_TEXTURE = 5,  /* MonoTextureValue  {texture_coordinates=b (vector input), texture=a, output (number)} :47-51 */
    PYR_OP_RGB_SPECTRUM = 6,  /* RgbSpectrumValue{wavelength=x, source=a (rgb reg), output}  :52-56 */
    PYR_OP_FRESNEL = 7,       /* Fresnel {ior=x, env_ior=y, normal=a, incident=b (vector inputs), output} :57-63 */
    PYR_OP_BLACKBODY = 8,     /* Blackbody {wavelength=x, temperature=y, output}             :64-68 */
    PYR_OP_RGB_TO_VECTOR = 9, /* Convert::RgbToVector {source=a, output}                     :69-71,104-110 */
    PYR_OP_BINARY = 10,       /* Binary {value_type, operator, lhs=a, rhs=b, output}         :72-78 */
    PYR_OP_MIX = 11,          /* Mix {value_type, lhs=a, rhs=b, amount=x, output}            :79-85 */
    PYR_OP_CLAMP = 12         /* Clamp {value=x, min=y, max=z, output}                       :86-91 */
} PyrOp;

typedef enum PyrValueType { PYR_VT_NUMBER = 0, PYR_VT_VECTOR = 1, PYR_VT_RGB = 2 } PyrValueType; /* :112-118 */
typedef enum PyrBinaryOperator { PYR_BIN_ADD = 0, PYR_BIN_SUB = 1, PYR_BIN_MUL = 2, PYR_BIN_DIV = 3 } PyrBinaryOperator;

/* NumberValue<N> (instruction.rs:94-99). */
typedef enum PyrOperandKind { PYR_OPERAND_CONSTANT = 0, PYR_OPERAND_INPUT = 1, PYR_OPERAND_REGISTER = 2 } PyrOperandKind;
typedef enum PyrNumberInput { PYR_INPUT_WAVELENGTH = 0 } PyrNumberInput;                 /* program/mod.rs:117-120 */
typedef enum PyrVectorInput { PYR_INPUT_NORMAL = 0, PYR_INPUT_INCIDENT = 1, PYR_INPUT_TEXTURE = 2 } PyrVectorInput; /* :130-135 */

/* Inputs bitflags (program/mod.rs:150-159). */
#define PYR_DEP_WAVELENGTH 0x01u
#define PYR_DEP_NORMAL 0x10u
#define PYR_DEP_INCIDENT 0x20u
#define PYR_DEP_TEXTURE 0x40u

typedef struct PyrOperand {
    uint32_t kind; /* PyrOperandKind */
    uint32_t bits; /* CONSTANT: the f32 bit pattern; INPUT: PyrNumberInput; REGISTER: number register */
} PyrOperand;

typedef struct PyrInstr {
    uint32_t op;         /* PyrOp */
    uint32_t value_type; /* PyrValueType, BINARY / MIX only */
    uint32_t operator_;  /* PyrBinaryOperator, BINARY only */
    uint32_t deps;       /* Instruction::dependencies (instruction.rs:15): the inputs the instruction depends on, through the registers it reads
                          * too. For a path's further wavelengths only the PYR_DEP_WAVELENGTH instructions run again, over the registers the
                          * first run left (program/memoized.rs): a caller's program must compute the same value under both runs. */
    uint32_t output;     /* register index; the register file follows from op / value_type */
    uint32_t a;
    uint32_t b;
    uint32_t reserved;
    PyrOperand x, y, z, w;
} PyrInstr; /* 64 bytes */

/* The size of the interpreter's in-register file, not a limit on programs. pyr_scene_create renumbers the registers of a program
 * that declares more (pyr_program_allocate_registers); a program that still needs more after that runs on the wide interpreter
 * build, whose file holds PYR_WIDE_*_REGISTERS, and one that needs more than that is refused with
 * PYR_ERR_UNSUPPORTED. A program may declare at most PYR_MAX_DECLARED_REGISTERS registers of each file (both front ends keep that
 * bound; pyr_scene_create and pyr_program_allocate_registers refuse more with PYR_ERR_UNSUPPORTED). */
#define PYR_MAX_NUMBER_REGISTERS 16
#define PYR_MAX_VECTOR_REGISTERS 8
#define PYR_MAX_RGB_REGISTERS 8
#define PYR_WIDE_NUMBER_REGISTERS 64
#define PYR_WIDE_VECTOR_REGISTERS 32
#define PYR_WIDE_RGB_REGISTERS 32
#define PYR_MAX_DECLARED_REGISTERS 65536

/* ProgramType (program/mod.rs:61-73): Constant short-circuits, Instructions reads one output register. */
typedef enum PyrProgramKind { PYR_PROGRAM_CONSTANT = 0, PYR_PROGRAM_INSTRUCTIONS = 1 } PyrProgramKind;
typedef enum PyrProgramOutput { PYR_OUTPUT_NUMBER = 0, PYR_OUTPUT_VECTOR = 1 } PyrProgramOutput; /* mod.rs:103-106 */

typedef struct PyrProgram {
    uint32_t kind;        /* PyrProgramKind */
    float constant;       /* value of a Constant program */
    uint32_t first_instr; /* into PyrSceneDesc::instrs */
    uint32_t num_instrs;
    uint32_t output_kind; /* PyrProgramOutput */
    uint32_t output_reg;
    uint32_t num_numbers; /* register counts: program/mod.rs:67-71 */
    uint32_t num_vectors;
    uint32_t num_rgbs;
} PyrProgram;

/* Spectrum<f32> (project/spectra.rs:13-24). ARRAY: `count` samples evenly spaced over [min,max],
 * clamped to the end values outside (spectra.rs:32-55). CURVE: `count` (x,y) pairs (2*count floats),
 * zero at and outside the end points (math.rs:22-72). Data lives at spectrum_data[offset...]. */
typedef enum PyrSpectrumFormat { PYR_SPECTRUM_ARRAY = 0, PYR_SPECTRUM_CURVE = 1 } PyrSpectrumFormat;
typedef struct PyrSpectrum {
    uint32_t format;
    float min;
    float max;
    uint32_t offset;
    uint32_t count;
} PyrSpectrum;

/* ---------------------------------------------------------------- materials ------------------- */

/* SurfaceBsdfType (materials/mod.rs:336-342). */
typedef enum PyrBsdf { PYR_BSDF_EMISSIVE = 0, PYR_BSDF_DIFFUSE = 1, PYR_BSDF_MIRROR = 2, PYR_BSDF_REFRACTIVE = 3 } PyrBsdf;

/* MaterialComponent (materials/mod.rs:230-235) + refractive::Properties (refractive.rs:39-45). */
typedef struct PyrComponent {
    uint32_t bsdf;                /* PyrBsdf */
    uint32_t color_program;       /* SurfaceBsdf::color */
    int32_t probability_program;  /* -1 = None */
    float selection_compensation; /* = number of entries in the list this component belongs to (mod.rs:213-221) */
    float ior, env_ior, dispersion, env_dispersion;
} PyrComponent;

/* Material {surface{components, emissive}, normal_map} (materials/mod.rs:27-31, :83-87). The emissive
 * list holds its own copies (with their own selection_compensation) of the emissive components. */
typedef struct PyrMaterial {
    uint32_t first_component;
    uint32_t num_components;
    uint32_t first_emissive;
    uint32_t num_emissive;
    int32_t normal_map_program; /* -1 = None; else a program with vector output run on NormalInput (materials/mod.rs:68-80) */
} PyrMaterial;

/* Texture<LinSrgba> / Texture<LinLuma> (texture.rs:18-22): linearised texels, row-major from the top row of the image
 * (texture.rs:163: data[x + y * width]). Color textures hold (red, green, blue, alpha), mono textures one luma value. */
typedef enum PyrTextureFormat { PYR_TEXTURE_COLOR = 0, PYR_TEXTURE_MONO = 1 } PyrTextureFormat;
typedef struct PyrTexture {
    uint32_t format; /* PyrTextureFormat */
    uint32_t width, height;
    uint32_t reserved;
    uint64_t offset; /* first texel's float in PyrSceneDesc.texture_data */
} PyrTexture;

/* Lamp (lamp.rs:12-20). */
typedef enum PyrLampKind { PYR_LAMP_DIRECTIONAL = 0, PYR_LAMP_POINT = 1, PYR_LAMP_SHAPE = 2 } PyrLampKind;
typedef enum PyrShapeKind { PYR_SHAPE_SPHERE = 0, PYR_SHAPE_TRIANGLE = 1, PYR_SHAPE_PLANE = 2 } PyrShapeKind;
typedef struct PyrLamp {
    uint32_t kind;          /* PyrLampKind */
    uint32_t shape_kind;    /* SHAPE: PyrShapeKind (sphere or triangle) */
    uint32_t shape_index;   /* SHAPE: index into the sphere / triangle arrays */
    uint32_t color_program; /* DIRECTIONAL / POINT */
    float v[3];             /* DIRECTIONAL: direction (as given, not normalised); POINT: position */
    float width;            /* DIRECTIONAL: cosine of the half angle (lamp.rs:30-34, tracer.rs:452) */
} PyrLamp;

/* ---------------------------------------------------------------- the scene ------------------- */

/* World {sky, lights, planes, finite_objects} (world.rs:31-36) + Resources.spectra (program/mod.rs:144-148),
 * after World::from_project (world.rs:39-271) has applied mesh scale and transform. */
typedef struct PyrSceneDesc {
    /* Shape::Triangle (shapes/mod.rs:39-46): v1,v2,v3 positions, unit vertex normals, uvs. */
    uint32_t num_triangles;
    const float* tri_positions;   /* [num_triangles][3][3] */
    const float* tri_normals;     /* [num_triangles][3][3] */
    const float* tri_uvs;         /* [num_triangles][3][2] or NULL (all zero) */
    const uint32_t* tri_material; /* [num_triangles] */

    /* Shape::Sphere (shapes/mod.rs:33-38). */
    uint32_t num_spheres;
    const float* spheres;           /* [num_spheres][4] = centre xyz, radius */
    const float* sphere_tex_scale;  /* [num_spheres][2] or NULL (1,1) */
    const uint32_t* sphere_material;

    /* shapes::Plane (shapes/mod.rs:434-439): point on the plane, unit normal, texture scale. */
    uint32_t num_planes;
    const float* planes; /* [num_planes][8] = origin xyz, normal xyz, texture_scale xy */
    const uint32_t* plane_material;

    uint32_t num_lamps;
    const PyrLamp* lamps; /* order == World::lights, pick_lamp indexes it (world.rs:301-305) */

    uint32_t num_materials;
    const PyrMaterial* materials;
    uint32_t num_components;
    const PyrComponent* components;

    uint32_t num_programs;
    const PyrProgram* programs;
    uint32_t num_instrs;
    const PyrInstr* instrs;

    uint32_t num_spectra;
    const PyrSpectrum* spectra;
    uint32_t num_spectrum_floats;
    const float* spectrum_data;

    /* crate::rgb::response::RGB (build.rs:18-59): `rgb_basis_count` rows of (r,g,b), an ARRAY spectrum over
     * [rgb_basis_min, rgb_basis_max]. NULL unless a program holds PYR_OP_RGB_SPECTRUM. */
    const float* rgb_basis;
    uint32_t rgb_basis_count;
    float rgb_basis_min;
    float rgb_basis_max;

    uint32_t sky_program; /* World::sky */

    /* Resources.textures (project/textures.rs:13-16); PYR_OP_COLOR_TEXTURE / PYR_OP_MONO_TEXTURE index this one list. */
    uint32_t num_textures;
    const PyrTexture* textures;
    uint64_t num_texture_floats;
    const float* texture_data;

    /* Normal::from_space (shapes/mod.rs:531-535), the tangent-space rotation as a quaternion (s, x, y, z), after
     * make_triangle (world.rs:308-374) and Shape::transform (shapes/mod.rs:322-344). Needed for triangles whose material
     * has a normal map (NULL: identity) and for every plane (texture coordinates come from it, shapes/mod.rs:454-468;
     * NULL: derived from the plane normal as world.rs:88-100 does). Sphere frames are computed at the hit. */
    const float* tri_frames;   /* [num_triangles][3][4] or NULL */
    const float* plane_frames; /* [num_planes][4] or NULL */
} PyrSceneDesc;

typedef struct PyrScene PyrScene;

/* == Progress {progress: u8, message} (renderer/mod.rs:229-232). */
typedef void (*PyrProgressFn)(void* user, uint8_t percent, const char* message);

/* Work counters of one render (flags & PYR_FLAG_COUNTERS) -- the units SURVEY.md section 8(d) prices. */
typedef struct PyrCounters {
    uint64_t samples;         /* iterations of the simple.rs:78 loop */
    uint64_t extension_rays;  /* World::intersect calls from tracer.rs:222 */
    uint64_t shadow_rays;     /* World::intersect calls from tracer.rs:381 */
    uint64_t box_tests;       /* AABBs slab-tested (32 B each) */
    uint64_t triangle_tests;  /* Moeller-Trumbore tests (36 B each) */
    uint64_t sphere_tests;    /* 16 B each */
    uint64_t plane_tests;     /* 16 B each */
    uint64_t shaded_hits;     /* surface-data fetches (52 B each) */
    uint64_t exposures;       /* Film::expose calls that landed in the window (16 B each) */
} PyrCounters;

/* One closest-hit result of pyr_scene_intersect: == Intersection {distance, surface_point} (shapes/mod.rs:472-482). */
#define PYR_HIT_NONE 0xFFFFFFFFu
typedef struct PyrHit {
    float distance;
    uint32_t shape; /* PYR_HIT_NONE, or (PyrShapeKind << 30) | index */
    float u, v;     /* triangle barycentrics (ShapeSurfacePoint::Triangle {u, v}), else 0 */
} PyrHit;

/* ---------------------------------------------------------------- entry points ---------------- */

int pyr_abi_version(void);

/* Number of gfx950 devices visible to the process (0 if none; never fails). */
int pyr_device_count(void);

/* Thread-local description of the last error returned on this thread ("" if none). */
const char* pyr_last_error(void);

/* Replaces the part of World::from_project that builds the acceleration structure
 * (Bvh::new, world.rs:262 / spatial/bvh.rs:13-155) and freezes the scene: copies the description, builds the
 * BVH on the host, uploads everything to `device`.
 *   Sizes: fewer than 2^28 triangles + spheres; the kernels address a node by a 32-bit byte offset, so an acceleration
 * structure of 4 GB (2^26 binary nodes, about 200 M triangles) or more is refused with PYR_ERR_UNSUPPORTED rather than
 * wrapped around. A render call takes fewer than 2^32 pixels (and, as tile blocks, fewer than 2^32 block pixels), at most
 * 64 wavelengths per sample and fewer than 2^32 chunks of 64 samples; larger calls are refused the same way. */
int pyr_scene_create(const PyrSceneDesc* desc, int device, PyrScene** out_scene);
void pyr_scene_destroy(PyrScene* scene);

/* Replaces Renderer::render / simple::render (renderer/mod.rs:77-111, renderer/simple.rs:17-56) for
 * Algorithm::Simple. Blocking. Adds the exposures of this call into `film_inout`, a HOST buffer of
 * (film_row_count or height) * width * bins grains in the film.rs:56 layout. `on_status` may be NULL. */
int pyr_render_simple(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* params,
                      PyrGrain* film_inout, PyrProgressFn on_status, void* user);

/* Same, but `film_device` is DEVICE memory on the scene's device and the work is enqueued on `hip_stream`
 * (a hipStream_t, NULL = default stream) without synchronising: the caller synchronises the stream.
 * A PyrScene owns device-side working memory (counters, the spectral tape) that serves one render at a
 * time: renders of ONE scene must be issued on one stream (or otherwise ordered); different scenes are independent. A scene serves
 * one PyrSession or one plain render at a time (see "progressive sessions"). */
int pyr_render_simple_device(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film,
                             const PyrRenderParams* params, PyrGrain* film_device, void* hip_stream);

/* Counters of the last render on this scene that ran with PYR_FLAG_COUNTERS (synchronises the device). */
int pyr_scene_counters(PyrScene* scene, PyrCounters* out);

/* World::intersect (world.rs:273-299) for a batch of rays: rays = [n][6] (origin xyz, direction xyz), HOST memory;
 * hits = [n], HOST memory. `elapsed_ms`, if not NULL, receives the kernel's duration measured with HIP events;
 * `counters`, if not NULL, receives box/triangle/sphere/plane test counts for the batch (instrumented build). */
int pyr_scene_intersect(PyrScene* scene, const float* rays, uint32_t n, PyrHit* hits, float* elapsed_ms,
                        PyrCounters* counters);

/* Same for rays and hits already resident on the device, enqueued on `hip_stream` without synchronising. */
int pyr_scene_intersect_device(PyrScene* scene, const float* rays_device, uint32_t n, PyrHit* hits_device,
                               void* hip_stream);

/* Introspection of the acceleration structure the library built (node count, bytes, depth). */
typedef struct PyrBvhInfo {
    uint32_t num_nodes;   /* 64-byte two-child nodes */
    uint32_t num_leaves;
    uint32_t max_depth;
    uint32_t num_primitives;
    uint64_t node_bytes;
    uint64_t primitive_bytes;
    /* ABI 4: the tree the resumable traversal walks on scenes that do not live in LDS (0 when the scene has none): 128-byte
     * four-child nodes; for triangle-only scenes a second copy of them whose leaves index 80-byte records of two triangles */
    uint32_t num_wide_nodes;
    uint32_t num_pair_records;
    uint64_t wide_node_bytes;
    uint64_t pair_record_bytes;
} PyrBvhInfo;
int pyr_scene_bvh_info(PyrScene* scene, PyrBvhInfo* out);

/* ---- who builds the acceleration structure. pyr_scene_create builds the binary tree on one host thread (binned SAH, 16 bins on
 * three axes). pyr_scene_create_with may ask for the same tree from the device instead: level-synchronous binned SAH with the host
 * builder's rules, expression for expression, so that where no node needs the median fallback (median_splits == 0 below) the
 * tree is the host's -- the same nodes in the same order, the same PyrBvhInfo, the same hits and the same traversal counts; the
 * order of the up to four primitives inside a leaf is the only freedom (the device builder stores them ascending by shape code).
 * A node whose centroids cannot be separated by bins (coincident centroids, or the depth rule) is split at the median: the device
 * gives slot 0 the count / 2 references smallest by (centroid on the widest axis, shape code), which is deterministic but may
 * break ties differently from the host builder -- a valid tree of the same shape, possibly other leaves.
 *   The collapse to four-child nodes, the pair records and the upload are the host's in both cases. The device builder steps
 * aside, and the host builds, when spatial splits are asked for (PYRITE_SPATIAL_SPLITS=1) or when the scene is beyond what it
 * handles; PyrBuildInfo says so. Two builds of one scene give the same bytes, whoever builds. */
#define PYR_BUILD_HOST 0u
#define PYR_BUILD_DEVICE 1u
typedef struct PyrBuildParams {
    uint32_t builder;     /* PYR_BUILD_HOST or PYR_BUILD_DEVICE */
    uint32_t reserved[7]; /* zero */
} PyrBuildParams;
/* pyr_scene_create with a choice of builder. `build` NULL: exactly pyr_scene_create. An unknown `builder` or a non-zero reserved
 * word is PYR_ERR_INVALID_ARGUMENT, reported before the description is looked at and before any device is touched. */
int pyr_scene_create_with(const PyrSceneDesc* desc, int device, const PyrBuildParams* build, PyrScene** out_scene);

#define PYR_BUILD_FALLBACK_NONE 0u
#define PYR_BUILD_FALLBACK_SPATIAL_SPLITS 1u    /* PYRITE_SPATIAL_SPLITS=1 and the scene gets a pair tree: only the host splits space */
#define PYR_BUILD_FALLBACK_MEDIAN_TOO_LARGE 2u  /* a node of more than 2048 references needed the median rule */
#define PYR_BUILD_FALLBACK_INTERNAL 3u          /* the device's result did not pass the host's validation, or nodes were left after the
                                                   last level the depth rule allows (never expected) */
/* How a scene's acceleration structure was built, for host-built scenes too. Times are host wall-clock milliseconds of the
 * stages of scene creation: the primitives' bounds; the binary tree (device builder: upload, every level, download; when it
 * stepped aside, its attempt and the host build); its finishing pass (device builder only: renumbering into the host builder's
 * layout); the collapse to four-child nodes; everything else (packing, pair records, upload); and all of scene creation. `reserved`
 * is always 0. The digest is no part of scene creation: the first pyr_scene_build_info of a scene walks the binary tree, which the
 * scene keeps on the host until then (64 bytes per node and 4 per primitive) and frees afterwards; later calls return the same value.
 * `tree_digest`: a pre-order walk of the binary tree hashing each child's stored box (-0.0f read as +0.0f), depth and slot, and a
 * leaf's shape codes sorted -- node numbers and the order inside a leaf do not enter, so equal digests mean the same tree. */
typedef struct PyrBuildInfo {
    uint32_t builder_asked, builder_used; /* differ when the device builder stepped aside */
    uint32_t fallback_reason;             /* PYR_BUILD_FALLBACK_* */
    uint32_t levels;                      /* iterations of the device builder's level loop (0: built on the host) */
    uint32_t median_splits;               /* nodes split by the median rule: 0 means the tree is tie-free */
    uint32_t reserved;
    uint64_t tree_digest;
    float bounds_ms, tree_ms, finish_ms, collapse_ms, pack_upload_ms, total_ms;
} PyrBuildInfo;
int pyr_scene_build_info(PyrScene* scene, PyrBuildInfo* out);

/* ---- moving a live scene's geometry. A PyrScene is no longer frozen where its primitives are: pyr_scene_update takes new
 * positions for the SAME primitives and leaves the scene ready to render again, without repeating register allocation, the
 * product split, the texture upload or -- for a refit -- the tree build.
 *   What may change: where things are. Counts, materials, uvs, planes, programs, textures and the lamp list do not change; an
 * array left NULL stays as the scene holds it (positions without normals: a pure translation).
 *   Argument checks and atomicity: a NULL update, an unknown mode, a non-zero reserved word, an array given for a count of zero,
 * a NULL scene and counts that are not the scene's are PYR_ERR_INVALID_ARGUMENT, in that order, before any device is looked for;
 * pyr_last_error names the argument. The new arrays pass the coordinate check of scene creation ("Coordinates": 1e15 units,
 * finite; PYR_ERR_UNSUPPORTED) before anything of the scene is written, so a refused update leaves the scene as it was.
 *   Live sessions: a scene counts its PyrSessions and refuses an update while there is one (PYR_ERR_INVALID_ARGUMENT): a session
 * renders from the scene whenever it is asked to. The one-render-at-a-time rule of the _device entry points covers
 * pyr_scene_update_device too: the caller orders it against this scene's other work on other streams.
 *   PYR_UPDATE_REBUILD builds a new tree with the scene's builder (host or device, as at creation): afterwards the scene is in
 * every observable respect the scene pyr_scene_create_with makes from the same description with the new arrays -- PyrBuildInfo
 * (digest included; its times are those of the rebuild), PyrBvhInfo, hits, traversal counters and films -- because it runs the
 * geometry part of scene creation again. Programs, materials, spectra and textures are neither touched nor uploaded again.
 *   PYR_UPDATE_REFIT keeps the topology: primitive order, leaf sizes and every count are those of the last build, and everything
 * derived from positions is new -- the primitive and pair records, the triangles' shading normals and texture frames, the sphere
 * table, the records of shape lamps (the arithmetic of scene creation, on the host) and every stored box of the binary, the
 * four-child and the pair tree. A leaf's box is the exact min / max of its primitives, moved outward by the padding of the NEW
 * bounds (16 ulps of the largest coordinate); an inner child's box is the union of that child's stored boxes, which is the padded
 * union because x - pad is monotone. So a refit with unchanged arrays reproduces the bytes creation uploaded, and two updates
 * with the same arrays write the same bytes. Empty slots and empty leaves keep their boxes. A scene built with
 * PYRITE_SPATIAL_SPLITS=1 holds clipped boxes: PYR_UPDATE_REFIT refuses it with PYR_ERR_UNSUPPORTED, PYR_UPDATE_REBUILD serves it.
 *   A refit never rebuilds by itself. PyrUpdateInfo::area_ratio is the caller's signal for when to ask for a rebuild.
 *   pyr_scene_build_info keeps describing the last build (creation or rebuild).
 *   pyr_scene_update reads HOST arrays and returns when the scene is ready. pyr_scene_update_device reads DEVICE arrays on the
 * scene's device (16-byte aligned) and enqueues its kernels on `hip_stream`; it copies the arrays to the host first (the
 * coordinate check, the lamp records and the description a later rebuild starts from live there), which waits for the stream. */
#define PYR_UPDATE_REFIT   0u  /* keep the tree's topology, recompute every box bottom-up */
#define PYR_UPDATE_REBUILD 1u  /* build a new tree with the scene's builder (host or device, as at creation) */
typedef struct PyrGeometryUpdate {
    uint32_t mode;
    uint32_t num_triangles, num_spheres;   /* must equal the scene's */
    const float* tri_positions;  /* [n][3][3] or NULL: triangles stay */
    const float* tri_normals;    /* [n][3][3] or NULL: normals stay (a pure translation) */
    const float* tri_frames;     /* [n][3][4] or NULL: frames stay */
    const float* spheres;        /* [n][4] or NULL */
    uint32_t reserved[4];
} PyrGeometryUpdate;
int pyr_scene_update(PyrScene*, const PyrGeometryUpdate*);                            /* HOST arrays, blocking */
int pyr_scene_update_device(PyrScene*, const PyrGeometryUpdate*, void* hip_stream);   /* DEVICE arrays on the scene's device */
/* The last update of a scene (all zero, area_ratio 1, before the first): the mode it ran, the launches of its longest refit
 * schedule (the binary tree's heights; 0 for a rebuild), how many updates the scene has taken since the last build, and host
 * wall-clock milliseconds -- new arrays to where the kernels read them (pyr_scene_update_device: to the host), the records,
 * the boxes, and the whole call. pyr_scene_update waits between the stages, so its times are the device's too;
 * pyr_scene_update_device's last two are the time to enqueue. A rebuild's bill is PyrBuildInfo's; here it is total_ms.
 * `area_ratio`: the sum of the half areas of every stored child box of the binary tree, now, over the same sum at the last
 * build, in f64 in node order -- 1.0 for a tree as built, larger as a refit loosens it. Computed on this call (it fetches the
 * binary tree), never on an update's bill. */
typedef struct PyrUpdateInfo { uint32_t mode_used, levels, updates; float upload_ms, prims_ms, refit_ms, total_ms; double area_ratio; uint32_t reserved[4]; } PyrUpdateInfo;
int pyr_scene_update_info(PyrScene*, PyrUpdateInfo* out);

/* ---- posing a live scene's objects. pyr_scene_update takes whole new arrays; most callers know less and more: WHICH object moves
 * and by WHAT matrix. pyr_scene_set_objects names contiguous primitive ranges as objects and keeps the scene's geometry at that
 * call on the device as the REST POSE; pyr_scene_pose takes one transform per object, computes every primitive of every object
 * from the rest pose on the device, and runs the refit (or the rebuild) of pyr_scene_update from there: 80 bytes per object
 * cross the bus instead of 120 bytes per triangle.
 *   pyr_scene_set_objects: the ranges must lie inside the scene's counts and be pairwise disjoint (PYR_ERR_INVALID_ARGUMENT
 * otherwise, as are a NULL scene and NULL ranges with a count); primitives in no range never move. Calling it again replaces the
 * ranges and captures the rest pose again (the geometry as it is then, posed or not); num_objects == 0 forgets the objects and
 * frees the rest pose. A pyr_scene_update[_device] that carries any array forgets them too -- those arrays are a new geometry,
 * not a pose of the old one -- and pyr_scene_pose is PYR_ERR_INVALID_ARGUMENT until objects are set again.
 *   pyr_scene_pose leaves the scene, in every observable respect, as pyr_scene_update (host arrays, the same mode) leaves it when
 * given the arrays P(rest, poses). P is the reference's Shape::scale, then Shape::transform with Normal::transform, applied to the
 * REST pose, never to the previous pose, all in f32 and unfused:
 *     triangles  position *= scale; every vertex normal n and frame q become n' = normalize(M3 n),
 *                q' = quat_from_cols(normalize(M3 (q * ex)), normalize(M3 (q * ey)), n'); then position = M position
 *                (normalize(v) = v * (1 / |v|), |v| = sqrt((x*x + y*y) + z*z); M3 = the upper 3x3 of `transform`)
 *     spheres    radius *= scale; centre *= scale; centre = M centre
 * The last row of `transform` must be exactly 0,0,0,1, so the reference's division by w is by exactly 1. An object whose pose is
 * exactly the identity matrix with scale 1.0f is COPIED from rest bit for bit (Normal::transform by the identity is not the
 * identity on bits).
 *   Argument checks, in this order, before any device is looked for (pyr_last_error names the argument): a NULL scene or update;
 * an unknown mode; a non-zero reserved word, in the update or in any pose; num_objects that is not the scene's, or no objects set;
 * NULL poses; a matrix entry or scale that is not finite; a last row that is not 0,0,0,1 -- all PYR_ERR_INVALID_ARGUMENT. A live
 * PyrSession and a refit of a spatial-split tree are refused as pyr_scene_update refuses them.
 *   Atomicity: the kernels write the posed arrays into the scene's staging arrays and touch no record; a bound of a moved primitive
 * that fails the coordinate check of scene creation ("Coordinates") sets one word, which the call reads back -- its only wait on
 * `hip_stream` before the refit is enqueued. Then the call returns PYR_ERR_UNSUPPORTED and the scene renders as before.
 *   Shape lamps get their records from the posed arrays on the device, with the arithmetic of scene creation.
 *   PYR_UPDATE_REBUILD poses on the device, fetches the posed arrays and runs the geometry part of scene creation, as
 * pyr_scene_update does; it serves spatial-split scenes. pyr_scene_update_info describes a pose too: upload_ms is the pose kernels
 * and the read-back of the word.
 *   pyr_scene_geometry copies the scene's geometry as it is now to HOST arrays ([n][3][3], [n][3][3], [n][3][4], [n][4]); a NULL
 * array is skipped, and tri_frames must be NULL for a scene created without frames. It waits for the device. */
typedef struct PyrObjectRange { uint32_t first_triangle, num_triangles, first_sphere, num_spheres; } PyrObjectRange;
int pyr_scene_set_objects(PyrScene*, const PyrObjectRange* ranges, uint32_t num_objects);
typedef struct PyrObjectPose {
    float transform[16];   /* column-major like PyrCamera::cam_to_world; last row 0,0,0,1 */
    float scale;           /* uniform, applied before the transform */
    uint32_t reserved[3];
} PyrObjectPose;
typedef struct PyrPoseUpdate {
    uint32_t mode;               /* PYR_UPDATE_REFIT | PYR_UPDATE_REBUILD */
    uint32_t num_objects;        /* must equal the scene's */
    const PyrObjectPose* poses;  /* HOST, [num_objects] */
    uint32_t reserved[4];
} PyrPoseUpdate;
int pyr_scene_pose(PyrScene*, const PyrPoseUpdate*, void* hip_stream);
int pyr_scene_geometry(PyrScene*, float* tri_positions, float* tri_normals, float* tri_frames, float* spheres);

/* ---- skinning a live scene's meshes. A pose moves an object as one rigid piece; a mesh that bends -- a figure on a skeleton, a
 * cable, a flag -- has a matrix per VERTEX, blended from a few joint matrices by weights that never change (linear blend skinning).
 * pyr_scene_set_skins takes those bindings once, 72 bytes per skinned triangle; pyr_scene_skin takes one small table of joint
 * matrices per frame (and, if wanted, the objects' poses), computes every triangle from the rest pose on the device and runs the
 * refit or the rebuild of pyr_scene_pose from there.
 *   A skin belongs to one object of pyr_scene_set_objects and covers all of that object's triangles, in their order; the object's
 * spheres are not skinned. For every vertex it names four joints j0..j3 (relative to the skin's first joint) and four weights
 * w0..w3. A frame supplies the skin's joint matrices J[0..num_joints), column-major like PyrObjectPose::transform, last row exactly
 * 0,0,0,1. The vertex's matrix B is blended per entry e of the upper three rows, unfused f32 in this order:
 *     B[e] = ((w0*J[j0][e] + w1*J[j1][e]) + w2*J[j2][e]) + w3*J[j3][e]          last row 0,0,0,1
 * and the vertex takes the per-vertex rule of pyr_scene_pose with transform B and scale 1.0f: position = B position,
 * n' = normalize(B3 n) (NOT an inverse transpose), frames as there. The object's own pose is then applied to the skinned vertex by
 * the same rule (skipped bit for bit when it is exactly the identity): the geometry is P_object(S(rest, bindings, J)), always from
 * rest, never from the previous frame. A skin whose joint matrices are ALL exactly the identity is copied from rest bit for bit,
 * the same convention as an identity pose (decided per skin on the host). Weights are not renormalised.
 *   pyr_scene_set_skins needs objects to be set. It copies the bindings to the device and sets every joint to the identity; the
 * geometry does not change at this call. num_skins == 0 forgets the skins. Every pyr_scene_set_objects call forgets them, and so
 * does every pyr_scene_update[_device] that carries an array: skins hang on objects, objects on the rest pose. Refused with
 * PYR_ERR_INVALID_ARGUMENT, in this order, before any device is looked for (pyr_last_error names the argument): NULL skins with a
 * non-zero count; a NULL scene; no objects set; a non-zero reserved word; an object index out of range; an object without
 * triangles; two skins on one object; num_joints 0 or above 65,536; NULL joints or weights; a joint index >= num_joints, even
 * under a zero weight; a weight that is not finite or is negative; a vertex whose weights, summed left to right in f32, are
 * further than 1e-3 from 1. A refused call leaves the previous skins in place.
 *   pyr_scene_skin is one call, one pose-and-skin pass, one read-back of the flag and one refit or rebuild; its contract is
 * pyr_scene_pose's: it leaves the scene as pyr_scene_update (host arrays, the same mode) leaves it when given the arrays above; a
 * bound beyond 1e15 is PYR_ERR_UNSUPPORTED and the scene renders as before; a live PyrSession and a refit of a spatial-split tree
 * are refused; shape lamps get their records from the staged arrays on the device; pyr_scene_update_info describes the call.
 * `poses` NULL: the objects keep the poses they are in (num_objects must still be the scene's). To pyr_scene_pose's argument
 * checks, in its order, it adds: no skins set; num_joints that is not the scene's (the skins' counts summed); NULL joints; an entry
 * that is not finite; a last row that is not 0,0,0,1. pyr_scene_pose on a scene with skins keeps the joints that scene is in. */
typedef struct PyrSkin {
    uint32_t object;          /* index into the ranges of pyr_scene_set_objects */
    uint32_t num_joints;      /* 1 .. 65,536 */
    const uint16_t* joints;   /* HOST, [object's num_triangles][3][4] */
    const float* weights;     /* HOST, [object's num_triangles][3][4] */
    uint32_t reserved[4];
} PyrSkin;
int pyr_scene_set_skins(PyrScene*, const PyrSkin* skins, uint32_t num_skins);
/* ---- dual quaternion skinning, chosen per skin. Where two joints twist against each other the linear blend above is no rotation
 * and the mesh loses volume (the "candy wrapper": joints 170 degrees apart about the bone leave the ring between them 9 % of its
 * radius). A dual-quaternion skin (Kavan et al. 2007) blends its joints as rigid motions instead; only how the vertex's matrix B is
 * made changes, and everything after B is the rule above. All f32 and unfused; normalize, sqrt and 1/x as in pyr_scene_pose;
 * dot4(a,b) = ((a0*b0 + a1*b1) + a2*b2) + a3*b3.
 *   Per joint, once per frame, on the host: r = quat_from_cols(c0, c1, c2) of the joint's upper 3x3 columns, (s,x,y,z);
 * k = 1/sqrt(dot4(r,r)); r = r*k per component. With t the translation column, the dual part d = 0.5 * (0,t) * r:
 *     d0 = -0.5f*((t0*r1 + t1*r2) + t2*r3)        d1 = 0.5f*((t0*r0 + t1*r3) - t2*r2)
 *     d2 =  0.5f*((t1*r0 + t2*r1) - t0*r3)        d3 = 0.5f*((t0*r2 + t2*r0) - t1*r1)
 * Q[j] = (r, d), eight floats, in a device table beside the twelve-float one, allocated and uploaded only while some skin is
 * dual-quaternion: a scene without such a skin allocates, uploads and launches nothing for it.
 *   Per vertex, on the device, with the binding's j0..j3 and w0..w3: the pivot is joint j0; for k = 1..3
 * wk' = dot4(r[j0], r[jk]) < 0 ? -wk : wk (a dot of zero or NaN does not negate), w0' = w0;
 *     b[e] = ((w0'*Q[j0][e] + w1'*Q[j1][e]) + w2'*Q[j2][e]) + w3'*Q[j3][e]          for the eight entries
 * s = dot4(b[0..4], b[0..4]); a lane with !(s >= 1e-30f && s <= 1e30f) raises bit 3 (value 8) of the call's flag word;
 * k = 1/sqrt(s); r = b[0..4]*k, d = b[4..8]*k; the translation t = 2 * (d * conj(r)):
 *     t0 = 2.0f*(((d1*r0 - d0*r1) - d2*r3) + d3*r2)
 *     t1 = 2.0f*(((d2*r0 - d0*r2) + d1*r3) - d3*r1)
 *     t2 = 2.0f*(((d3*r0 - d0*r3) - d1*r2) + d2*r1)
 * B's upper 3x3 is cgmath's Matrix3::from(Quaternion) of r = (s,x,y,z): with x2=x+x, y2=y+y, z2=z+z, xx2=x2*x, xy2=x2*y, xz2=x2*z,
 * yy2=y2*y, yz2=y2*z, zz2=z2*z, sx2=x2*s, sy2=y2*s, sz2=z2*s the columns are (1-yy2-zz2, xy2+sz2, xz2-sy2),
 * (xy2-sz2, 1-xx2-zz2, yz2+sx2), (xz2+sy2, yz2-sx2, 1-xx2-yy2); the fourth column is t, the last row 0,0,0,1. The vertex then takes
 * exactly what a linearly blended vertex takes: the per-vertex rule with transform B and scale 1.0f, then the object's pose. As
 * above: a skin whose joint matrices are all exactly the identity copies rest bit for bit, weights are not renormalised, an index
 * at or above the skin's count uses joint 0 and raises bit 0, and the geometry is always computed from rest.
 *   pyr_scene_set_skin_blend gives one mode per skin, in skin order. It needs skins to be set, sets every joint to the identity as
 * pyr_scene_set_skins does, and the geometry does not change at this call. pyr_scene_set_skins makes every skin linear again, and
 * whatever forgets the skins forgets the modes. Refused with PYR_ERR_INVALID_ARGUMENT, in this order, before any device is looked
 * for: NULL modes; a NULL scene; no skins set; num_skins that is not the scene's; an unknown mode. A refused call leaves the modes
 * as they were.
 *   pyr_scene_skin and pyr_scene_morph add one check, after "a last row that is not 0,0,0,1": a joint of a dual-quaternion skin whose
 * upper 3x3 is not a rotation is refused. A rotation here: |dot(ci,ci) - 1| <= 1e-3f for each column, |dot(ci,cj)| <= 1e-3f for
 * each pair, dot(cross(c0,c1), c2) > 0, with dot(a,b) = (a0*b0 + a1*b1) + a2*b2. The flag word: bits 0, 1 and 2 keep their order
 * and messages; bit 3 without any of them is PYR_ERR_UNSUPPORTED with a message that names a blended joint rotation (the rotations
 * of a vertex's joints cancel, as two antipodal ones under equal weights). The scene renders as before. */
#define PYR_SKIN_LINEAR 0u
#define PYR_SKIN_DUAL_QUATERNION 1u
int pyr_scene_set_skin_blend(PyrScene*, const uint32_t* modes, uint32_t num_skins);
typedef struct PyrSkinUpdate {
    uint32_t mode;               /* PYR_UPDATE_REFIT | PYR_UPDATE_REBUILD */
    uint32_t num_objects;        /* must equal the scene's */
    const PyrObjectPose* poses;  /* HOST, [num_objects], or NULL: the objects keep the poses they are in */
    const float* joints;         /* HOST, [num_joints][16], the skins' tables one after the other in skin order */
    uint32_t num_joints;         /* must equal the scene's: the skins' num_joints summed */
    uint32_t reserved[4];
} PyrSkinUpdate;
int pyr_scene_skin(PyrScene*, const PyrSkinUpdate*, void* hip_stream);

/* ---- morph targets for a live scene's meshes. A skin bends a mesh over a skeleton; a face that changes expression, a muscle that
 * bulges, a corrective shape at an elbow or a cloth cache played back between key shapes is a weighted sum of per-vertex deltas.
 * pyr_scene_set_morphs takes the deltas once, 36 bytes per target and triangle (72 with normal deltas); pyr_scene_morph takes one
 * weight per target per frame (and, if wanted, joint matrices and the objects' poses), computes every triangle from the rest pose on
 * the device and runs the refit or the rebuild of pyr_scene_pose from there.
 *   A morph belongs to one object of pyr_scene_set_objects and covers all of that object's triangles, in their order; the object's
 * spheres are not morphed. It has T targets, each a dense array of position deltas dp[t][triangle][vertex][3], and either all of its
 * targets have normal deltas dn of the same shape or none has. A frame supplies one weight w[t] per target. A target is ACTIVE
 * when w[t] != 0.0f (both zeros are inactive); an inactive target is skipped and its deltas are not read (adding 0 * d is not a
 * no-op on bits). A morph with no active target is AT REST: its triangles are the rest arrays bit for bit -- positions, normals
 * and frames -- decided per morph on the host, as with an identity skin. Otherwise, per vertex, all f32 and unfused, over the
 * active targets in ascending t:
 *     positions  p = p + w[t] * dp[t]                                    per component
 *     normals    (morph with normal deltas) m = n, then m = m + w[t] * dn[t]; s = (m.x*m.x + m.y*m.y) + m.z*m.z;
 *                n' = normalize(m)                                       (normalize as in pyr_scene_pose)
 *     frames     (scene that keeps frames) with dot(a,b) = (a0*b0 + a1*b1) + a2*b2, rx = q * ex, ry = q * ey:
 *                d = dot(rx, n'); x = rx - n'*d per component; x = normalize(x);
 *                e = dot(ry, n'); f = dot(ry, x); y = (ry - n'*e) - x*f per component; y = normalize(y);
 *                q' = quat_from_cols(x, y, n')       -- a Gram-Schmidt of the old tangent frame against the new normal
 * A squared length s that is normalised -- of m, of x, of y -- must lie in [1e-30, 1e30]: a lane with !(s >= 1e-30f && s <= 1e30f)
 * raises bit 1 of the call's flag word (below). A morph without normal deltas keeps rest's normals and frames bit for bit.
 *   The morphed vertex then takes what its object already has: the skin rule of pyr_scene_skin if the object has a skin, and the
 * object's pose on top, each skipped bit for bit under the conventions stated there. The geometry is
 * P_object(S(M(rest, targets, w), bindings, J)), always from rest, never from the previous frame. Weights may be negative or above
 * 1 and are not renormalised.
 *   pyr_scene_set_morphs needs objects to be set. It copies the deltas to the device, in morph order, keeps a device copy of the rest
 * positions, normals and frames that the morph is written into, and sets every weight to 0; the geometry does not change at this
 * call. num_morphs == 0 forgets the morphs. Every pyr_scene_set_objects call forgets them, and so does every
 * pyr_scene_update[_device] that carries an array; pyr_scene_set_skins and pyr_scene_set_morphs each leave the other's state in
 * place. Refused with PYR_ERR_INVALID_ARGUMENT, in this order, before any device is looked for (pyr_last_error names the
 * argument): NULL morphs with a non-zero count; a NULL scene; no objects set; a non-zero reserved word; an object index out of
 * range; an object without triangles; two morphs on one object; num_targets 0 or above 256; NULL position_deltas; a delta that is
 * not finite. A refused call leaves the previous morphs in place.
 *   pyr_scene_morph is pyr_scene_skin with a weight table: one call, one morph-pose-and-skin pass, one read-back of the flag word
 * and one refit or rebuild, with pyr_scene_pose's contract and atomicity. `poses`, `joints` and `weights` may each be NULL: the
 * scene keeps what it is in. The flag word: bit 0 (a bound beyond 1e15, which a morphed position that is not finite fails too) is
 * PYR_ERR_UNSUPPORTED with pyr_scene_pose's message; bit 1 alone is PYR_ERR_UNSUPPORTED with a message that names a morphed normal;
 * either way the scene renders as before, under the weights, joints and poses it was in. Argument checks: pyr_scene_pose's, in its
 * order, with NULL poses allowed; then no morphs set; joints given on a scene without skins; for joints that are given,
 * pyr_scene_skin's checks of the table; num_weights that is not the scene's (the morphs' num_targets summed) when weights are
 * given; a weight that is not finite. pyr_scene_pose and pyr_scene_skin on a scene with morphs keep the weights it is in. */
typedef struct PyrMorph {
    uint32_t object;               /* index into the ranges of pyr_scene_set_objects */
    uint32_t num_targets;          /* 1 .. 256 */
    const float* position_deltas;  /* HOST, [num_targets][object's num_triangles][3][3] */
    const float* normal_deltas;    /* HOST, same shape, or NULL: normals and frames stay rest's */
    uint32_t reserved[4];
} PyrMorph;
int pyr_scene_set_morphs(PyrScene*, const PyrMorph* morphs, uint32_t num_morphs);
typedef struct PyrMorphUpdate {
    uint32_t mode;               /* PYR_UPDATE_REFIT | PYR_UPDATE_REBUILD */
    uint32_t num_objects;        /* must equal the scene's */
    const PyrObjectPose* poses;  /* HOST or NULL: keep */
    const float* joints;         /* HOST [num_joints][16] or NULL: keep (then num_joints is not read) */
    uint32_t num_joints;
    const float* weights;        /* HOST [num_weights], the morphs' targets one after the other in morph order; or NULL: keep */
    uint32_t num_weights;        /* must equal the scene's when weights is given */
    uint32_t reserved[4];
} PyrMorphUpdate;
int pyr_scene_morph(PyrScene*, const PyrMorphUpdate*, void* hip_stream);

/* ---- smooth normals for a live scene's meshes. A pose, a joint matrix and a morph carry the rest pose's shading normals along:
 * normalize(M3 n) under a matrix (no inverse transpose), rest's own bits under a morph without normal deltas. Neither is the normal
 * of the surface where it now is: a sheared, bulged or non-uniformly scaled mesh is shaded as if it still had its rest shape.
 * pyr_scene_set_smoothing takes, once, which corners of an object share a vertex; from then on every pyr_scene_pose, pyr_scene_skin
 * and pyr_scene_morph recomputes that object's vertex normals on the device from the positions the call has just computed, and
 * rebuilds the tangent frames against them. There is no per-frame call of its own and nothing crosses the bus per frame.
 *   A smoothing belongs to one object of pyr_scene_set_objects and covers all of that object's triangles, in their order; the
 * object's spheres are not touched. vertex_ids gives one label per corner, [triangle][3], arbitrary uint32_t values: the corners
 * of the object with equal labels form a GROUP and share one normal. Groups never cross objects (equal labels in two objects are
 * two groups). A crease is kept by giving its two sides different labels.
 *   Orientation, decided once at pyr_scene_set_smoothing from the rest pose (the arrays pyr_scene_set_objects captured, not a
 * morphed rest), all f32 and unfused: per triangle c = cross(p1 - p0, p2 - p0) with cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2,
 * a0*b1 - a1*b0); per component r = (n0 + n1) + n2 over its three rest normals; d = (c.x*r.x + c.y*r.y) + c.z*r.z. The triangle
 * is NEGATED iff d < 0 (a d of zero or NaN does not negate): it is wound against its normals.
 *   Per frame, after the morph, the skin and the pose have written the positions P of the call:
 *     face vector  c = cross(p1 - p0, p2 - p0) from the triangle's final positions, every component negated (-c) if the triangle
 *                  is negated; its length is twice the triangle's area, so the sum below is area-weighted
 *     group sum    over the group's corners in ascending corner index 3*triangle + k: m = c of the first corner's triangle (not
 *                  0 + c: 0 + (-0) loses a sign bit), then m = m + c per component for each further corner. A triangle that has
 *                  two corners in one group counts twice.
 *     normal       every corner of the group gets n' = normalize(m)           (normalize as in pyr_scene_pose)
 *     frames       (scene that keeps frames) the corner's frame as the call computed it -- morphed, skinned and posed -- is
 *                  Gram-Schmidt'ed against n' exactly as pyr_scene_set_morphs states for a morphed normal: x first, then y,
 *                  q' = quat_from_cols(x, y, n')
 * A squared length s that is normalised -- of m, of x, of y -- must lie in [1e-30, 1e30]: a lane with !(s >= 1e-30f && s <= 1e30f)
 * raises bit 2 (value 4) of the call's flag word.
 *   A smoothed object's normals and frames are ALWAYS N(final positions) after any pyr_scene_pose, pyr_scene_skin or
 * pyr_scene_morph, also under an identity pose, an identity skin and a morph at rest: positions are rest's bits there, normals the
 * recomputed ones. The geometry is N(P_object(S(M(rest)))). An object without a smoothing keeps those calls' own normals in
 * every word. pyr_scene_set_smoothing itself moves nothing: the geometry does not change at this call.
 *   pyr_scene_set_smoothing needs objects to be set. It packs the groups (4 bytes per corner and 4 per group on the device).
 * num_smoothings == 0 forgets the smoothing. Every pyr_scene_set_objects call forgets it, and so does every
 * pyr_scene_update[_device] that carries an array; pyr_scene_set_skins, pyr_scene_set_morphs and pyr_scene_set_smoothing leave each
 * other's state in place. Refused with PYR_ERR_INVALID_ARGUMENT, in this order, before any device is looked for (pyr_last_error
 * names the argument): NULL smoothings with a non-zero count; a NULL scene; no objects set; a non-zero reserved word; an object
 * index out of range; an object without triangles; two smoothings on one object; NULL vertex_ids. A refused call leaves the
 * previous smoothing in place.
 *   The flag word of pyr_scene_pose, pyr_scene_skin and pyr_scene_morph: bit 0 keeps its message and comes first; bit 1 keeps its
 * message; bit 2 without either is PYR_ERR_UNSUPPORTED with a message that names a recomputed normal (a group whose face vectors
 * cancel or vanish, as under a pose of scale 0). In every case the scene renders as before. */
typedef struct PyrSmoothing {
    uint32_t object;              /* index into the ranges of pyr_scene_set_objects */
    uint32_t reserved0;
    const uint32_t* vertex_ids;   /* HOST, [object's num_triangles][3]; equal labels share a normal */
    uint32_t reserved[4];
} PyrSmoothing;
int pyr_scene_set_smoothing(PyrScene*, const PyrSmoothing*, uint32_t num_smoothings);

/* Introspection of the kernel a render of `scene` with `params` would run (nothing is launched; only spectrum_samples is read
 * today). Results never depend on it -- every schedule is the same per-sample arithmetic as tracer.rs:208-345 -- but throughput
 * does, and a maintainer wants to see why a scene is slow: */
typedef struct PyrPathInfo {
    uint32_t stage_scheduler; /* 0: the bounce-synchronous walk (scenes that live in LDS and run no interpreter programs); 1: the
                                 stage-scheduled state machine */
    uint32_t interpreter;     /* 1: some program of the scene is not a constant / spectrum / one of the fast shapes: the kernel
                                 carries the program interpreter (and texture / normal-map sampling) */
    uint32_t scene_in_lds;    /* 1: nodes and primitives are staged in LDS */
    uint32_t tape;            /* 0: every wavelength's throughput is kept online; 1: spectral tape (no interpreter programs);
                                 2: hit tape -- interpreter programs run once per hit, the per-wavelength part is replayed at
                                 full width; needs spectrum_samples >= 4 and a tape form for every colour program (a product
                                 of a mono texture and a spectrum has none) */
    uint32_t phase_lanes;     /* lanes of a wave that must want a phase before it runs (stage scheduler; 0 otherwise) */
    uint32_t reserved[3];
} PyrPathInfo;
int pyr_scene_path_info(PyrScene* scene, const PyrRenderParams* params, PyrPathInfo* out);

/* The register files of a scene's programs (what pyr_scene_create made of them; nothing is launched). Largest counts over every
 * PYR_PROGRAM_INSTRUCTIONS program, as declared and after pyr_program_allocate_registers: */
typedef struct PyrProgramInfo {
    uint32_t declared_numbers, declared_vectors, declared_rgbs;
    uint32_t allocated_numbers, allocated_vectors, allocated_rgbs;
    uint32_t wide;     /* 1: some program needs more than the in-register file even after allocation: the scene runs the wide
                          interpreter build (PYR_WIDE_*_REGISTERS), without a tape (PyrPathInfo::tape 0) */
    uint32_t reserved;
} PyrProgramInfo;
int pyr_scene_program_info(PyrScene* scene, PyrProgramInfo* out);

/* Register allocation of one program, host only (no device needed): exactly the pass pyr_scene_create applies to every
 * PYR_PROGRAM_INSTRUCTIONS program that declares more than PYR_MAX_NUMBER_REGISTERS / PYR_MAX_VECTOR_REGISTERS /
 * PYR_MAX_RGB_REGISTERS. `instrs` and `instrs_out` are indexed like PyrSceneDesc::instrs: the pass reads
 * instrs[program->first_instr, + num_instrs) and writes the same range of instrs_out (which may be `instrs`); *program_out is
 * *program with output_reg and the three counts renumbered. Only register indices change -- the same instructions in the same
 * order, ops, deps, constants and inputs -- and the counts never grow. Linear scan, one pool per file; a value that does not
 * depend on the wavelength but is read by an instruction that does, and such a program output, keep a register of their own for
 * the whole program (the kernels re-run only the PYR_DEP_WAVELENGTH instructions for the companion wavelengths). A program that
 * fits the in-register file, a constant program and one the pass cannot follow (a register written twice, or read before it is
 * written or beyond its declared count) are copied unchanged. Deterministic. PYR_OK; PYR_ERR_INVALID_ARGUMENT for null pointers;
 * PYR_ERR_UNSUPPORTED (nothing written) for a program that declares more than PYR_MAX_DECLARED_REGISTERS registers of a file.
 * pyr_scene_create reads every program from the caller's instructions and gives a renumbered one a copy of its own, so programs
 * may share instruction ranges. */
int pyr_program_allocate_registers(const PyrInstr* instrs, const PyrProgram* program, PyrInstr* instrs_out, PyrProgram* program_out);

/* ---------------------------------------------------------------- multi-GPU -----------
 * The reference is one process with shared memory; its unit of parallel work is the tile (renderer/simple.rs:36-55: every
 * tile has its own RNG and exposes its own pixels, renderer/mod.rs:125-189 hands tiles to worker threads). Here the scene
 * is replicated on every GPU, the tiles of the image are dealt round-robin to the ranks (rank r of n renders tiles
 * r, r + n, ...: every rank sees every part of the image, which balances the cost without measuring it), every rank
 * renders its tiles in ONE launch into a private PYR_FILM_TILE_BLOCKS buffer with no data-path collective, and ONE gather
 * -- a group of ncclSend / ncclRecv over xGMI (RCCL) -- brings the blocks to rank 0, which adds them into the film.
 * With the per-(tile, iteration) RNG the n-GPU film equals the 1-GPU film up to the order of the float additions. */

/* Grains a PYR_FILM_TILE_BLOCKS buffer needs for the tiles `params` selects (tile_begin / tile_end / tile_stride /
 * tile_size); 0 when the arguments are invalid. */
uint64_t pyr_film_blocks_grains(const PyrFilmDesc* film, const PyrRenderParams* params);

/* Adds the blocks a render with these `params` (film_layout = PYR_FILM_TILE_BLOCKS) produced into `film_device`, a
 * whole-image film in the film.rs:56 layout; both buffers on `device`, enqueued on `hip_stream`. Ring pixels outside the
 * image do not exist and are skipped (nothing was exposed there). */
int pyr_film_blocks_assemble_device(const PyrFilmDesc* film, const PyrRenderParams* params, const PyrGrain* blocks_device,
                                    PyrGrain* film_device, int device, void* hip_stream);

/* One process per GPU (torch.distributed, MPI, ...): a communicator over RCCL. Rank 0 obtains an id with
 * pyr_comm_unique_id (ncclGetUniqueId; 128 bytes), the host brings it to the other ranks by whatever means it has, and
 * every rank calls pyr_comm_create (ncclCommInitRank) with its device. librccl is loaded when the first of these is
 * called; single-GPU use of the library never touches it. */
#define PYR_COMM_ID_BYTES 128
typedef struct PyrComm PyrComm;
int pyr_comm_unique_id(uint8_t id_out[PYR_COMM_ID_BYTES]);
/* A world of one rank needs no RCCL communicator and gets none -- unless the environment says PYRITE_FORCE_RCCL=1: then
 * ncclCommInitRank(nranks = 1) really runs and the rank's blocks travel through a grouped self ncclSend / ncclRecv, which
 * exercises the gather's code on a single GPU. pyr_comm_uses_rccl tells which kind a communicator is (1 / 0). */
int pyr_comm_create(const uint8_t id[PYR_COMM_ID_BYTES], int rank, int num_ranks, int device, PyrComm** out_comm);
int pyr_comm_uses_rccl(const PyrComm* comm);
void pyr_comm_destroy(PyrComm* comm);

/* This rank's part of a sharded render, enqueued on `hip_stream`: of the tiles `params` selects (normally all:
 * tile_begin = tile_end = 0, tile_stride <= 1) rank r renders every num_ranks-th starting at the r-th, sends its blocks
 * to rank 0 (grouped ncclSend / ncclRecv: the one gather), and rank 0 adds everybody's blocks into `film_device_rank0` (a
 * whole-image film on rank 0's device; ignored on the other ranks, may be NULL there). `scene` must live on the
 * communicator's device. Working buffers are kept on the communicator between calls.
 *   Failures up to the gather never leave a peer blocked (the reference's workers report to one collecting thread,
 * renderer/mod.rs:181-183): before anything is sent the ranks agree -- one one-word ncclAllReduce, waited for on the host -- that every rank got
 * through its argument checks and buffer growth; if one did not, EVERY rank returns an error and nothing is rendered. What
 * fails later (a launch, or the kernels flagging their own film invalid) travels in a trailer grain behind each rank's
 * blocks, so every rank still enters the gather; pyr_comm_status() reports it on rank 0 (every rank's trailer) and on the
 * sender (its own) once `hip_stream` has been waited for: PYR_OK, or PYR_ERR_DEVICE naming the rank -- the film is invalid
 * then. An error inside the collective calls themselves aborts THIS rank's communicator (ncclCommAbort); every later call on
 * it fails. pyr_render_simple_multi then aborts the sibling ranks' communicators too, at once, so none of its threads stays
 * in the gather; ranks in OTHER processes cannot be reached from here -- their wait on `hip_stream` ends when RCCL notices
 * the lost peer, so a multi-process caller should bound that wait.
 *   Coordinates: the kernels' normalize / square root are the correctly rounded IEEE results (the reference's) for lengths whose
 * squares are normal f32 numbers; pyr_scene_create refuses (PYR_ERR_UNSUPPORTED) a scene with a primitive beyond 1e15 units
 * from the origin, and features below ~1e-15 units are outside the verified range (the reference itself ignores anything
 * under DIST_EPSILON = 1e-4, math.rs:4). */
int pyr_comm_status(PyrComm* comm);
int pyr_render_simple_sharded(PyrComm* comm, PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film,
                              const PyrRenderParams* params, PyrGrain* film_device_rank0, void* hip_stream);

/* One process driving several GPUs (what a Rust host does with its thread pool): `scenes[i]` is the scene created on
 * the i-th device to use. Blocking; one host thread per device; the same plan and the same gather as above
 * (ncclCommInitAll). Adds the exposures into `film_inout`, a HOST film of the whole image. If the same device appears
 * more than once (a test rig: several logical ranks on one GPU, which RCCL refuses) the blocks travel by
 * hipMemcpyPeerAsync instead. `on_status` (may be NULL) is called on the calling thread only. */
int pyr_render_simple_multi(PyrScene* const* scenes, uint32_t num_devices, const PyrCamera* camera, const PyrFilmDesc* film,
                            const PyrRenderParams* params, PyrGrain* film_inout, PyrProgressFn on_status, void* user);

/* ---------------------------------------------------------------- film development ("next" row f1) -------------
 * The step after the hot path: main.rs:315-327 turns every developed pixel spectrum into an 8-bit sRGB pixel through
 * spectrum_to_xyz (main.rs:352-369: trapezoid rule over the film's wavelength span in `step_size` steps against the
 * CIE 1931 observer tables, divided by the span, times 3.444) and palette's Xyz -> linear sRGB -> sRGB encoding.
 * The optional `filter` and `white` programs of the project's image settings (main.rs:197-238) act on the sampled
 * intensity as  ((intensity * filter[i]) / white_div[i]) * white_mul[i]  at the i-th sampling wavelength
 * wl_i = wl_start + i*step_size (i = 0 .. sample_count-1); the host evaluates those programs once per wavelength and
 * passes the three arrays (NULL = stage absent).
 * As in the reference, the LAST pixel of the film is never developed (film.rs:299 `end < len`) and stays black. */
typedef struct PyrDevelopParams {
    float step_size;         /* 2.0 for the final image, 30.0 for previews (main.rs:270, :311) */
    float xyz_scale;         /* 3.444 (main.rs:368) */
    uint32_t sample_count;   /* number of sampling wavelengths = trapezoid steps + 1 */
    const float* filter;     /* [sample_count] or NULL */
    const float* white_div;  /* [sample_count] or NULL: max(white(wl)/white_max, 1e-6) */
    const float* white_mul;  /* [sample_count] or NULL: D65(wl)/D65_max */
    const float* xyz_table;  /* [xyz_count][3]: crate::xyz::response::{X,Y,Z} (build.rs:68-121), ARRAY spectra over [xyz_min, xyz_max] */
    uint32_t xyz_count;
    float xyz_min, xyz_max;
} PyrDevelopParams;

/* film: HOST grains of the whole image (height*width*bins); rgb_out: HOST, height*width*3 bytes, row-major RGB. Blocking. */
int pyr_film_develop(const PyrFilmDesc* film, const PyrGrain* grains, const PyrDevelopParams* params, uint8_t* rgb_out, int device);
/* Same with the film and the output resident on `device`; the PyrDevelopParams arrays stay HOST pointers (copied by the
 * call); enqueued on `hip_stream`. */
int pyr_film_develop_device(const PyrFilmDesc* film, const PyrGrain* grains_device, const PyrDevelopParams* params, uint8_t* rgb_device,
                            int device, void* hip_stream);

/* ---------------------------------------------------------------- progressive sessions (ABI 5) ----------------
 * main.rs:243-305 renders while a status closure rewrites a preview image from the live film every 20 s or more
 * (main.rs:261-299, developed with step_size = 30). pyr_render_simple is one call whose film is valid when it returns; a
 * PyrSession is the same render cut into passes: pass j renders the sample window [done, done + n) of every pixel's budget
 * (PyrRenderParams::sample_begin), so every pass covers the whole image and after the last one the film is the one-shot film up to
 * the order of the float additions. The session owns the film ON THE SCENE'S DEVICE, a stream of its own, the camera, the film
 * description and the renderer parameters; a preview develops the film there and brings only width*height*3 bytes to the host.
 *   A PyrScene serves ONE session or ONE plain render at a time (its working memory is one render's): do not render the
 * scene by other means, or through a second session, between a session's first pyr_session_render and the pyr_session_sync (or
 * preview / film / noise call, which all wait) that follows its last. The scene must outlive the session. One GPU: the
 * multi-GPU entries have no session form.
 *   PYR_SESSION_HALVES keeps two films A and B: pass number j (from 0) exposes into A when j is even and into B when j is odd. The
 * film of the session is then A + B (accs added, weights added), and pyr_session_noise compares the two. */
#define PYR_SESSION_HALVES 1u
typedef struct PyrSession PyrSession;

/* `params->pixel_samples` is the whole budget; sample_begin must be 0, the film layout PYR_FILM_ROWS over the whole image, flags
 * without PYR_FLAG_COUNTERS. The film starts zeroed; if `film_host` (HOST, height*width*bins grains) is not NULL it is uploaded and
 * the session adds to it (into A when there are halves). Blocking. */
int pyr_session_create(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* params, uint32_t flags,
                       const PyrGrain* film_host, PyrSession** out_session);
/* Waits for the session's stream first. NULL is a no-op. */
void pyr_session_destroy(PyrSession* session);
/* Enqueues one pass -- the next `samples` (> 0) samples of every pixel, clipped to the budget -- on the session's stream and
 * returns without waiting. PYR_OK and nothing done when the budget is spent. */
int pyr_session_render(PyrSession* session, uint32_t samples);
/* Waits for every pass enqueued so far; reports, as pyr_render_simple does, a render that flagged its own film invalid. */
int pyr_session_sync(PyrSession* session);
/* Samples per pixel of the passes enqueued so far (never more than the budget). */
int pyr_session_samples_done(PyrSession* session, uint32_t* out_samples);
/* The film as it stands after every pass enqueued so far, developed on the device (pyr_film_develop's arithmetic and bytes; with
 * halves, of A + B): rgb_out = HOST, height*width*3 bytes. Blocking; the film itself does not cross the bus. */
int pyr_session_preview(PyrSession* session, const PyrDevelopParams* develop_params, uint8_t* rgb_out);
/* The film after every pass enqueued so far, in the film.rs:56 layout (A + B with halves): HOST / DEVICE memory (the scene's
 * device) of height*width*bins grains. Both block. */
int pyr_session_film(PyrSession* session, PyrGrain* film_out);
int pyr_session_film_device(PyrSession* session, PyrGrain* film_out_device);
/* The two half films (PYR_SESSION_HALVES only), HOST memory of height*width*bins grains each. Blocking. */
int pyr_session_halves(PyrSession* session, PyrGrain* film_a_out, PyrGrain* film_b_out);
/* Noise estimate per tile of the make_tiles grid (renderer/algorithm.rs:152-188), raster order: out_per_tile = HOST,
 * tiles_x*tiles_y floats. Needs PYR_SESSION_HALVES and at least two passes (else PYR_ERR_INVALID_ARGUMENT). With a, b the f32
 * quotients acc/weight of a grain in A and in B (0 where the weight is 0), over every (pixel, bin) of the tile and summed in f64:
 *     value = sqrt( sum (a - b)^2 / sum ((a + b)/2)^2 ),   0 when the denominator is 0.
 * It is the relative RMS difference of the two halves. HALF of it estimates the relative error of the summed film: the
 * difference of two independent halves has four times the variance of their mean. It weighs every grain alike, so paths that
 * dispersed (one wavelength per sample) and paths that did not (every wavelength of the sample) count alike, and it is only
 * as good as the halves are equal: render passes of one size, an even number of them. A film passed to pyr_session_create
 * sits in A alone and counts as difference. Deterministic: no atomics, the same bits on every call. Nothing here stops a
 * render by this number. Blocking. */
int pyr_session_noise(PyrSession* session, float* out_per_tile);

/* The drop-in for main.rs:243-305, blocking: renders `params->pixel_samples` samples per pixel in passes of `pass_samples`,
 * calls `on_status` (may be NULL) after every pass with percent = samples_done*100/budget, and -- when `on_preview` is not NULL --
 * develops the film with `preview_develop_params` after a pass once `preview_min_interval_s` seconds (>= 0; main.rs:261 uses 20)
 * have gone by since the last preview (since the start, for the first), and hands it over: rgb = height*width*3 bytes, valid
 * during the callback only. Both callbacks run on the calling thread. At the end `film_inout` (HOST) holds what it held
 * plus the render's exposures, as with pyr_render_simple. */
typedef void (*PyrPreviewFn)(void* user, const uint8_t* rgb, uint32_t width, uint32_t height, uint32_t samples_done);
int pyr_render_simple_progressive(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* params,
                                  PyrGrain* film_inout, uint32_t pass_samples, PyrProgressFn on_status, PyrPreviewFn on_preview,
                                  double preview_min_interval_s, const PyrDevelopParams* preview_develop_params, void* user);

/* ---------------------------------------------------------------- first-hit feature images ---------------------
 * The noise-free description of what the camera sees, one record and one albedo spectrum per pixel: what a denoiser, a stopping
 * rule or a user who checks a scene before a long render reads. The reference has no such output; every step is one of its own:
 *   - pixel (x, y) takes grid x grid sub-samples; sub-sample j = jy*grid + jx sits at fx = (jx + 0.5f) / grid, fy = (jy + 0.5f) / grid
 *     of the pixel's view-plane rectangle (from, size) = Camera::to_view_area(x, y, 1, 1) (cameras.rs:57-68): px = from.x + size.x*fx,
 *     py = from.y + size.y*fy, unfused f32;
 *   - the ray is Camera::ray_towards(px, py) (cameras.rs:70-97) with `aperture` read as 0: the lens is its centre, nothing is drawn
 *     from an RNG, the pass is a pure function of its arguments (lens blur is not reproduced);
 *   - the hit is World::intersect (world.rs:273-299), the hit pyr_scene_intersect reports for that ray; surface data is
 *     SurfacePoint::get_surface_data (shapes/mod.rs:484-494), the shading normal Material::apply_normal_map (materials/mod.rs:68-80)
 *     run at the wavelength wl_start + wl_width * 0.5f with incident = the ray's direction;
 *   - albedo: bin b of fp->albedo_bins stands for wl_b = wl_start + ((float)b + 0.5f) * (wl_width / (float)albedo_bins). With N =
 *     the hit material's num_components, a = (sum over the components whose bsdf is not PYR_BSDF_EMISSIVE, in list order, of
 *     get_probability(c) * color_c) / (float)N, both programs run on {wl_b, shading normal, ray direction, texture coordinates};
 *     get_probability = probability_program * selection_compensation, or selection_compensation alone (materials/mod.rs:238-248).
 *     Every sub-sample adds a (0 on a miss) to the grain's acc and 1 to its weight, in sub-sample order: the developed albedo is
 *     anti-aliased against black. Emission and the sky have no channel;
 *   - the record: `normal` = the sum of the shading normals of the sub-samples that hit, in sub-sample order, divided by their
 *     number (not renormalised; 0 without a hit); `depth` = the mean PyrHit::distance of those; `coverage` = hits / grid^2; `shape` =
 *     PyrHit::shape of sub-sample grid*grid/2 (PYR_HIT_NONE on a miss) and `material` that hit's material index (0xFFFFFFFF).
 * Deterministic: a pixel is summed by one lane in a fixed order and written with plain stores, no float atomics; two calls write
 * the same bytes. One GPU; scenes that need the wide interpreter build are served. */
typedef struct PyrFeatureParams {
    uint32_t grid;        /* 1..8: grid x grid sub-samples per pixel */
    uint32_t albedo_bins; /* 1..64; read only when an albedo buffer is given */
    uint32_t reserved[2];
} PyrFeatureParams;
typedef struct PyrFeaturePixel {
    float normal[3];
    float depth;
    float coverage;
    uint32_t shape;
    uint32_t material;
    uint32_t reserved; /* 0 */
} PyrFeaturePixel; /* 32 bytes */

/* HOST buffers; blocking. film->bins is ignored: the albedo film has fp->albedo_bins bins over film's wavelength span.
 * albedo_inout (height*width*albedo_bins grains in the film.rs:56 layout, added into) and pixels_out (height*width records,
 * row-major, overwritten) may each be NULL, not both. Arguments are checked before a device is looked for: PYR_ERR_INVALID_ARGUMENT
 * for a null pointer, a grid outside 1..8, albedo_bins outside 1..64 with an albedo buffer, an empty image or wavelength span, or
 * 2^32 pixels or more (pyr_last_error names the argument). */
int pyr_render_features(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrFeatureParams* fp,
                        PyrGrain* albedo_inout, PyrFeaturePixel* pixels_out);
/* Same with DEVICE buffers on the scene's device, enqueued on `hip_stream` without synchronising. The pass uses the scene's
 * working memory: the one-render-at-a-time rule of pyr_render_simple_device holds for it too. pixels_device must be 16-byte
 * aligned (hipMalloc's memory is; PYR_ERR_INVALID_ARGUMENT otherwise). */
int pyr_render_features_device(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrFeatureParams* fp,
                               PyrGrain* albedo_device, PyrFeaturePixel* pixels_device, void* hip_stream);
/* The session's camera and image size, on the session's stream, ordered after the passes enqueued so far; blocking. HOST outputs,
 * each may be NULL (not both); here the albedo is OVERWRITTEN: the pass runs into a zeroed film. The session's own film is not
 * touched, and further passes may follow. */
int pyr_session_features(PyrSession* session, const PyrFeatureParams* fp, PyrGrain* albedo_out, PyrFeaturePixel* pixels_out);

/* ---------------------------------------------------------------- linear images and tone mapping ---------------
 * pyr_film_develop ends in 8 bits behind a hard clamp (main.rs:315-327). These entries stop one step earlier and hand out the image
 * in linear light, three f32 per pixel, row-major: PYR_LINEAR_XYZ is spectrum_to_xyz's result after `xyz_scale`, PYR_LINEAR_SRGB
 * the linear sRGB triple the 8-bit path clamps and encodes -- the same operations in the same order, so the floats are the very
 * values pyr_film_develop encodes. The last pixel of the film is 0, 0, 0, as it is black there (film.rs:299). A second film
 * `grains_b` (NULL: none) is developed as grains + grains_b, accs added and weights added, the sum a session with halves holds.
 *
 * Statistics (of a linear sRGB image). Per pixel, in f32 and unfused:  Y = (0.2126f*R + 0.7152f*G) + 0.0722f*B.  A pixel is LIT
 * when Y > 0 and DARK otherwise (zero, negative, NaN). Lit pixels fill a histogram of 256 bins, 8 per octave over [2^-16, 2^16),
 * read off the bits of Y:  bin = clamp((int)(bits(Y) >> 20) - 888, 0, 255)  -- 888 = 111 << 3 is the biased exponent of 2^-16 with
 * three mantissa bits below it; smaller values (denormals too) fall into bin 0, larger ones and +inf into bin 255. Bin k ends below
 * upper_edge(k) = float_of_bits((k + 889) << 20). min_lit / max_lit are the extremes of Y over the lit pixels (0 when none is).
 * All counters are integers: the result does not depend on the order of the pixels and two calls give the same bits.
 *
 * Tone mapping (linear sRGB -> 8-bit sRGB), f32 and unfused, clamp(x) = fminf(fmaxf(x, 0), 1) (a NaN becomes 0):
 *   PYR_TONE_CLIP      v_c = clamp(exposure * c)                                   with exposure 1: pyr_film_develop to the byte
 *   PYR_TONE_REINHARD  a pixel that is not lit is black; else  L = exposure * Y,  Ld = (L * (1.0f + L / (white*white))) / (1.0f + L),
 *                      s = Ld / L,  v_c = clamp((exposure * c) * s)                extended Reinhard on luminance: L = white -> 1
 *   byte_c = (uint8)(e * 255.0f + 0.5f),  e = clamp(v <= 0.0031308f ? 12.92f*v : 1.055f*(float)pow((double)v, 1.0/2.4) - 0.055f)
 *
 * The automatic rule (pyr_tone_resolve, host arithmetic only). With target(p) = ceil((double)p * lit) clipped to 1..lit and
 * bin(p) = the first bin whose cumulative count reaches target(p):
 *   exposure <= 0:  exposure = key / upper_edge(bin(percentile))   -- the median luminance lands on `key`; 1 when nothing is lit
 *   white <= 0 (PYR_TONE_REINHARD only; PYR_TONE_CLIP does not read it and gets 1):
 *                   white = exposure * upper_edge(bin(white_percentile));           1 when nothing is lit
 * The usual values are key 0.18, percentile 0.5, white_percentile 0.99 (PYR_TONE_KEY, PYR_TONE_PERCENTILE, PYR_TONE_WHITE_PERCENTILE). */
#define PYR_LINEAR_XYZ 0u
#define PYR_LINEAR_SRGB 1u
#define PYR_TONE_CLIP 0u
#define PYR_TONE_REINHARD 1u
#define PYR_TONE_KEY 0.18f
#define PYR_TONE_PERCENTILE 0.5f
#define PYR_TONE_WHITE_PERCENTILE 0.99f
typedef struct PyrImageStats {
    uint32_t histogram[256];
    uint32_t lit, dark;
    float min_lit, max_lit;
} PyrImageStats; /* 1040 bytes */
typedef struct PyrToneParams {
    uint32_t op;            /* PYR_TONE_CLIP or PYR_TONE_REINHARD */
    float exposure;         /* a factor on the linear values; <= 0: automatic */
    float white;            /* the exposed luminance that becomes 1 (PYR_TONE_REINHARD); <= 0: automatic */
    float key;              /* > 0, read when the exposure is automatic */
    float percentile;       /* in (0, 1] */
    float white_percentile; /* in (0, 1] */
} PyrToneParams;

/* Every entry below checks its arguments before it looks for a device: PYR_ERR_INVALID_ARGUMENT for a null pointer, an unknown
 * `space` or `op`, bad development parameters, a percentile outside (0, 1], a key that is not positive; PYR_ERR_UNSUPPORTED for an
 * image of more than 2^32 - 1 pixels (the counters are 32 bits wide); then PYR_ERR_DEVICE when there is no such device. */

/* HOST grains (grains_b may be NULL) -> HOST out, height*width*3 floats. Blocking. */
int pyr_film_develop_linear(const PyrFilmDesc* film, const PyrGrain* grains, const PyrGrain* grains_b, const PyrDevelopParams* params, uint32_t space,
                            float* out, int device);
/* Same with the films and the output resident on `device`, enqueued on `hip_stream` (the PyrDevelopParams arrays stay HOST pointers). */
int pyr_film_develop_linear_device(const PyrFilmDesc* film, const PyrGrain* grains_device, const PyrGrain* grains_b_device, const PyrDevelopParams* params,
                                   uint32_t space, float* out_device, int device, void* hip_stream);
/* linear_srgb: HOST, height*width*3 floats; out: HOST. Blocking. */
int pyr_image_stats(const float* linear_srgb, uint32_t width, uint32_t height, PyrImageStats* out, int device);
/* Both buffers on `device`; enqueued on `hip_stream`, `out_device` is valid in stream order. */
int pyr_image_stats_device(const float* linear_srgb_device, uint32_t width, uint32_t height, PyrImageStats* out_device, int device, void* hip_stream);
/* The automatic rule above; no device is touched. `stats` may be NULL when nothing is automatic. Writes the exposure and the white
 * point pyr_image_tonemap is to be called with. */
int pyr_tone_resolve(const PyrImageStats* stats, const PyrToneParams* tone, float* exposure_out, float* white_out);
/* `resolved`: exposure > 0 and, for PYR_TONE_REINHARD, white > 0 (else PYR_ERR_INVALID_ARGUMENT); key and the percentiles are not
 * read. HOST buffers, rgb_out = height*width*3 bytes. Blocking. */
int pyr_image_tonemap(const float* linear_srgb, uint32_t width, uint32_t height, const PyrToneParams* resolved, uint8_t* rgb_out, int device);
int pyr_image_tonemap_device(const float* linear_srgb_device, uint32_t width, uint32_t height, const PyrToneParams* resolved, uint8_t* rgb_device, int device,
                             void* hip_stream);
/* The session's film as it stands after every pass enqueued so far (A + B with halves), developed to a linear image on the session's
 * stream: out = HOST, height*width*3 floats. Blocking. */
int pyr_session_linear(PyrSession* session, const PyrDevelopParams* develop_params, uint32_t space, float* out);
/* pyr_session_preview with a tone curve: linear sRGB development, statistics (only when something is automatic or they are asked
 * for), pyr_tone_resolve, tone mapping -- all on the session's stream and device. rgb_out = HOST, height*width*3 bytes; stats_out
 * (HOST) may be NULL. The linear image does not cross the bus. Blocking. */
int pyr_session_preview_tone(PyrSession* session, const PyrDevelopParams* develop_params, const PyrToneParams* tone, uint8_t* rgb_out,
                             PyrImageStats* stats_out);

/* ---------------------------------------------------------------- denoising a linear image from two halves -------
 * A session with PYR_SESSION_HALVES holds two films of independent samples, and development is linear in the grain quotients: the
 * two developed halves are two independent estimates of one image. These entries filter such a pair -- three f32 per pixel, never
 * the film -- with a non-local-means cross filter: the weights that average half `a` are read from half `b` and the other way
 * round, so the noise of a pixel never votes for itself. The reference has no such step.
 *   Inputs: `a`, `b`: width*height*3 f32, row-major, the halves. Optional guides, NULL = absent: `albedo`, width*height*3 f32 (the
 * albedo film of the feature pass developed to linear sRGB), and `pixels`, width*height PyrFeaturePixel records (normal, depth).
 *   All arithmetic is f32 and unfused, one rounding per operation, sums in the order written and started from 0.0f. p, q are
 * pixels, c a channel (0, 1, 2 in this order wherever channels are summed), "inside" means inside the image.
 *
 * Variance of one half:  s_c(p) = (a_c(p) - b_c(p))^2;  V_c(p) = 0.5f * (sum / (float)count), the sum of s_c over p's 3 x 3
 * neighbourhood clipped to the image in raster order (rows outer), count the pixels summed (4, 6 or 9; 1, 2 or 3 on a thin image).
 * Where that value is +inf, V_c(p) is NaN: an infinite pixel then poisons every term it enters, as a NaN one does by itself.
 *
 * Colour distance of p and q = p + o read from half H: t runs over the (2*patch+1)^2 patch offsets in raster order, dy outer, dx
 * inner, channel innermost. An offset t is skipped when p + t or q + t is not inside; n counts the offsets kept (t = 0 always is).
 *     S = sum ((H_c(p+t) - H_c(q+t))^2 - (V_c(p+t) + fminf(V_c(p+t), V_c(q+t)))) / (epsilon + (k*k) * (V_c(p+t) + V_c(q+t)))
 *     D = fmaxf(S / (3.0f * (float)n), 0.0f)
 * (the difference is squared as d*d, k*k is one product formed once). Guides, each only when its buffer is given and its sigma is
 * positive, in this order, with g the guide's term:  D = fmaxf(D, g),
 *     albedo: g = (sum_c (alb_c(p) - alb_c(q))^2) / (2.0f * (sigma_albedo * sigma_albedo))
 *     normal: the same form with PyrFeaturePixel::normal and sigma_normal
 *     depth:  z = PyrFeaturePixel::depth, m = fmaxf(fmaxf(z_p, z_q), 1e-30f), r = (z_p - z_q) / m,
 *             g = (r*r) / (2.0f * (sigma_depth * sigma_depth))
 * A pixel without coverage has normal 0 and depth 0 and needs no special case.
 *
 * Weight:  w(p, q) = expf(-D).  NaN: C's fmaxf drops a NaN operand, so the rule is explicit: w = 0 when S / (3.0f * (float)n) or a
 * guide term that applies is NaN. w(p, p) = 1 by definition, nothing is computed for o = 0. An offset whose q is not inside is
 * skipped, and an offset whose weight is 0 adds nothing to either sum below (0 * NaN would be NaN). Together: a NaN or infinite
 * pixel of either half makes V NaN in its 3 x 3 neighbourhood, every pair that touches it gets weight 0, the pixel keeps its own
 * value and gives it to nobody, and the pixels within patch + 1 of it come back as (a + b) * 0.5f, unfiltered.
 *
 * Cross filtering, o over the (2*radius+1)^2 window in raster order (oy outer), w_B the weights read from H = b:
 *     FA_c(p) = (sum_o w_B(p, p+o) * a_c(p+o)) / (sum_o w_B(p, p+o));   FB the same with the halves exchanged.
 * Outputs:  out = (FA + FB) * 0.5f;  error_out (optional) = fabsf(FA - FB) * 0.5f, the noise that is left, per pixel and channel.
 * Only expf is not pinned to the bit here. Deterministic: one lane owns a pixel, there are no float atomics, two calls write
 * the same bytes.
 *   The variance assumes halves of equal sample counts: as with pyr_session_noise, render passes of one size and an even number
 * of them. Halves of unequal size bias V -- the noisier half is under-estimated, the other over-estimated -- and with it every
 * weight. Nothing is filtered per wavelength bin, across GPUs, over time or twice. */
#define PYR_DENOISE_RADIUS 5u
#define PYR_DENOISE_PATCH 1u
#define PYR_DENOISE_K 0.45f
#define PYR_DENOISE_EPSILON 1e-10f
#define PYR_DENOISE_SIGMA_ALBEDO 0.02f
#define PYR_DENOISE_SIGMA_NORMAL 0.1f
#define PYR_DENOISE_SIGMA_DEPTH 0.02f
#define PYR_DENOISE_MAX_RADIUS 10u
#define PYR_DENOISE_MAX_PATCH 3u
typedef struct PyrDenoiseParams {
    uint32_t radius;      /* 1..PYR_DENOISE_MAX_RADIUS: the window is (2*radius+1)^2 pixels */
    uint32_t patch;       /* 0..PYR_DENOISE_MAX_PATCH: the patch is (2*patch+1)^2 pixels */
    float k;              /* > 0: smaller keeps more detail and more noise */
    float epsilon;        /* > 0 */
    float sigma_albedo;   /* <= 0 turns that guide off */
    float sigma_normal;
    float sigma_depth;
    uint32_t reserved;    /* 0 */
} PyrDenoiseParams; /* 32 bytes */

/* Arguments are checked before a device is looked for: PYR_ERR_INVALID_ARGUMENT, with the argument named in pyr_last_error, for a
 * null a, b, params or out, an empty image, radius, patch, k or epsilon out of range (a NaN is out of range), a non-zero reserved
 * word; PYR_ERR_UNSUPPORTED for more than 2^32 - 1 pixels; only then PYR_ERR_DEVICE when there is no such device.
 * HOST buffers; albedo, pixels and error_out may be NULL. Blocking. */
int pyr_image_denoise(const float* a, const float* b, const float* albedo, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height,
                      const PyrDenoiseParams* params, float* out, float* error_out, int device);
/* The same with every buffer resident on `device`, enqueued on `hip_stream`; out and error_out may not overlap the inputs. The
 * working memory (three images of width*height*3 floats) is allocated and freed in stream order. */
int pyr_image_denoise_device(const float* a_device, const float* b_device, const float* albedo_device, const PyrFeaturePixel* pixels_device, uint32_t width,
                             uint32_t height, const PyrDenoiseParams* params, float* out_device, float* error_out_device, int device, void* hip_stream);
/* The session's two half films, each developed to linear sRGB with `develop_params` (pyr_film_develop_linear of A alone and of B
 * alone), then denoised, all on the session's stream and device: out = HOST, height*width*3 floats; error_out (HOST) may be NULL.
 * With `feature_params` (NULL: no guides) the feature pass runs first into a zeroed albedo film of feature_params->albedo_bins bins,
 * that film is developed with the same `develop_params`, and it and the feature records guide the filter. Needs PYR_SESSION_HALVES
 * and at least two passes (else PYR_ERR_INVALID_ARGUMENT, as pyr_session_noise); the remark on halves of unequal size above holds.
 * The session's films are not touched, and further passes may follow. Blocking. */
int pyr_session_denoised(PyrSession* session, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params,
                         const PyrDenoiseParams* denoise_params, float* out, float* error_out);

/* ---------------------------------------------------------------- motion records and accumulation over frames ----
 * A scene moves between frames (pyr_scene_update, pyr_scene_pose, pyr_scene_skin) and so may the camera. The motion pass answers,
 * per pixel: where was the surface point this pixel sees one frame ago, and how far from the previous camera? pyr_image_reproject
 * is the simplest consumer of the answer, a running mean of linear images that follows the surfaces. The reference has neither.
 *
 * The previous frame's geometry. pyr_scene_keep_previous(scene, keep != 0) copies the scene's triangle positions ([n][3][3]) and
 * its sphere table ([n][4]) AS THEY ARE NOW into a snapshot on the scene's device: 36 bytes a triangle, 16 a sphere, both in the
 * description's primitive order, the one PyrHit::shape indexes. Blocking. A second call replaces the snapshot, keep == 0 frees
 * it, pyr_scene_destroy frees it. It survives every later pyr_scene_update / _pose / _skin in either mode: counts never change in
 * a scene's life and the indices are the description's, so a rebuild does not invalidate it. The call only reads the scene: a
 * live PyrSession does not forbid it. A NULL scene is PYR_ERR_INVALID_ARGUMENT, before a device is looked for.
 *
 * The pass takes one ray per pixel: sub-sample 0 of grid = 1 of the feature pass, the pixel centre through the centre of the lens.
 * `shape` and `depth` are therefore, bit for bit, those of pyr_render_features with grid = 1. No material program runs.
 *   All arithmetic is f32 and unfused, one rounding per operation, in the order written; sqrt is the correctly rounded one. The
 * hit is (t, shape, u, v) = PyrHit of the ray (o, d), P the position the surface data of that hit has: o + d*t on a triangle, the
 * point the sphere and the plane routine return otherwise. Q, where that material point was:
 *   triangle i, snapshot rows a, b, c:   e1 = b - a, e2 = c - a, Q = (a + e1*u) + e2*v, per component
 *   sphere i, now (c, r), snapshot (c', r'):   Q = c' + (P - c) * (r' / r)     -- a sphere's rotation is not tracked
 *   plane:   Q = P (planes never move);   no snapshot kept:   Q = P for every shape (only the camera moved)
 * Into the previous camera, W = pyr_camera_world_to_cam(previous_camera), column-major:
 *   q.x = ((W[0]*Q.x + W[4]*Q.y) + W[8]*Q.z) + W[12], q.y and q.z from rows 1 and 2 alike.
 * On a miss the direction d is a point at infinity: q.x = (W[0]*d.x + W[4]*d.y) + W[8]*d.z, depth = prev_depth = 0, HIT clear, and
 * the projection below still applies, so a sky follows a turning camera.
 *   zc = -q.z;  PYR_MOTION_IN_FRONT iff zc > 0, else prev_x = prev_y = 0 and INSIDE is clear. With vp = previous_camera->view_plane:
 *   vx = (q.x / zc) * vp,  vy = (-q.y / zc) * vp                       (the inverse of Camera::ray_towards, cameras.rs:78-81)
 *   m = fmaxf((float)width, (float)height) * 0.5f
 *   prev_x = vx*m + (float)width*0.5f,  prev_y = vy*m + (float)height*0.5f          (the inverse of to_view_area, cameras.rs:57-68)
 *   prev_depth = sqrt((q.x*q.x + q.y*q.y) + q.z*q.z) on a hit
 * focus_distance and aperture of the previous camera are not read. Deterministic: a lane owns a pixel and writes its record with
 * two 16-byte stores; two calls write the same bytes. One GPU. */
#define PYR_MOTION_HIT 1u      /* the ray hit something */
#define PYR_MOTION_IN_FRONT 2u /* the previous point lies in front of the previous camera */
#define PYR_MOTION_INSIDE 4u   /* and 0 <= prev_x < width, 0 <= prev_y < height */
typedef struct PyrMotionPixel {
    float prev_x, prev_y; /* continuous pixel coordinates in the previous frame (pixel centres at +0.5) */
    float prev_depth;     /* distance from the previous camera's origin to the previous point; 0 on a miss */
    float depth;          /* PyrHit::distance of this frame's ray; 0 on a miss */
    uint32_t shape;       /* PyrHit::shape, PYR_HIT_NONE on a miss */
    uint32_t flags;
    uint32_t reserved[2]; /* 0 */
} PyrMotionPixel; /* 32 bytes */

int pyr_scene_keep_previous(PyrScene* scene, int keep);
/* world_to_cam of a camera, host arithmetic only: the affine inverse of cam_to_world in f64 by cofactors, each entry rounded once
 * to f32, column-major, last row 0, 0, 0, 1. PYR_ERR_INVALID_ARGUMENT for a null pointer, an entry that is not finite, a last row
 * that is not exactly 0, 0, 0, 1, or a 3 x 3 determinant that is 0 or not finite. The motion entries call it themselves. */
int pyr_camera_world_to_cam(const PyrCamera* camera, float out[16]);
/* HOST pixels_out, height*width records, row-major; blocking. Of `film` only width and height are read. Arguments are checked before
 * a device is looked for: PYR_ERR_INVALID_ARGUMENT, with the argument named in pyr_last_error, for a null scene, camera,
 * previous_camera, film or pixels_out, an empty image, 2^32 pixels or more, a previous camera pyr_camera_world_to_cam refuses. */
int pyr_render_motion(PyrScene* scene, const PyrCamera* camera, const PyrCamera* previous_camera, const PyrFilmDesc* film, PyrMotionPixel* pixels_out);
/* Same with pixels_device on the scene's device (16-byte aligned, else PYR_ERR_INVALID_ARGUMENT), enqueued on `hip_stream` without
 * synchronising. The pass uses the scene's working memory: the one-render-at-a-time rule of pyr_render_simple_device holds. */
int pyr_render_motion_device(PyrScene* scene, const PyrCamera* camera, const PyrCamera* previous_camera, const PyrFilmDesc* film, PyrMotionPixel* pixels_device,
                             void* hip_stream);
/* The session's camera as the current one and its image size, on the session's stream after the passes enqueued so far; HOST
 * pixels_out; blocking. The session's film is not touched, and further passes may follow. */
int pyr_session_motion(PyrSession* session, const PyrCamera* previous_camera, PyrMotionPixel* pixels_out);

/* Accumulation over frames: out = the running mean of `current` and of the history fetched where each pixel's surface was.
 * `current`, `history`, `out`: width*height*3 f32 in linear light; `history_count`, `count_out`: one f32 a pixel, the frames the
 * pixel's mean holds; `motion`: this frame's records, `history_motion`: the records the history's frame was made with. The three
 * history buffers are all NULL (a first frame) or all given. No scene is needed. Per pixel with record r, f32 and unfused:
 *   No history -- out = current, count_out = 1 -- when there are no history buffers, PYR_MOTION_IN_FRONT is clear, or prev_x or
 *   prev_y is not finite. Else gx = r.prev_x - 0.5f, x0 = floorf(gx), fx = gx - x0, the same in y; four taps (x0, y0), (x0 + 1.0f, y0),
 *   (x0, y0 + 1.0f), (x0 + 1.0f, y0 + 1.0f) with weights (1.0f-fx)*(1.0f-fy), fx*(1.0f-fy), (1.0f-fx)*fy, fx*fy. A tap counts iff
 *   it lies inside the image (decided on the floats, before any cast), history_motion[tap].shape == r.shape, where r has
 *   PYR_MOTION_HIT  fabsf(h.depth - r.prev_depth) <= depth_tolerance * fmaxf(h.depth, r.prev_depth)  with h = history_motion[tap],
 *   history_count[tap] > 0, and the tap's three history floats are finite. Wt, Hc (per channel) and N are the sums over the counting
 *   taps, in tap order from 0.0f, of w, w * history_c and w * history_count. If Wt > 0 is false: no history, as above. Otherwise
 *   H_c = Hc / Wt, n = fminf(N / Wt, max_history), out_c = H_c + (current_c - H_c) / (n + 1.0f), count_out = n + 1.0f.
 * A surface that was hidden a frame ago finds no tap of its shape and depth and starts again at 1: the disocclusion rule. One lane
 * owns a pixel, there are no atomics, two calls write the same bytes. Nothing clamps the history to the neighbourhood of `current`,
 * nothing reads a variance, nothing jitters the pixel centre: pyr_image_temporal_resolve ("temporal resolve", below) does the first two. */
#define PYR_REPROJECT_DEPTH_TOLERANCE 0.02f /* = PYR_DENOISE_SIGMA_DEPTH */
#define PYR_REPROJECT_MAX_HISTORY 32.0f
typedef struct PyrReprojectParams {
    float depth_tolerance; /* >= 0, finite */
    float max_history;     /* >= 1, finite: the mean forgets older frames at the rate 1 / (max_history + 1) */
    uint32_t reserved[2];  /* 0 */
} PyrReprojectParams;
/* Arguments are checked before a device is looked for: PYR_ERR_INVALID_ARGUMENT, with the argument named in pyr_last_error, for a
 * null current, motion, params, out or count_out, history buffers of which some but not all are NULL, an empty image, parameters
 * out of range (a NaN is), a non-zero reserved word; PYR_ERR_UNSUPPORTED for more than 2^32 - 1 pixels; only then PYR_ERR_DEVICE.
 * HOST buffers. Blocking. */
int pyr_image_reproject(const float* current, const PyrMotionPixel* motion, const float* history, const PyrMotionPixel* history_motion, const float* history_count,
                        uint32_t width, uint32_t height, const PyrReprojectParams* params, float* out, float* count_out, int device);
/* The same with every buffer resident on `device`, enqueued on `hip_stream`; out and count_out may not overlap an input. The two
 * record arrays must be 16-byte aligned (hipMalloc's memory is; PYR_ERR_INVALID_ARGUMENT otherwise). */
int pyr_image_reproject_device(const float* current_device, const PyrMotionPixel* motion_device, const float* history_device,
                               const PyrMotionPixel* history_motion_device, const float* history_count_device, uint32_t width, uint32_t height,
                               const PyrReprojectParams* params, float* out_device, float* count_out_device, int device, void* hip_stream);

/* ---------------------------------------------------------------- motion blur over the motion records ----
 * A frame is an instantaneous still; this post filter spreads every pixel along the way its surface point went while the shutter
 * was open. It is the gather of McGuire, Hennessy, Bukowski and Osman, "A Reconstruction Filter for Plausible Motion Blur" (I3D
 * 2012), restated for the records above. It needs no scene. `image`, `out`: width*height*3 f32 in linear light; `motion`: the
 * records of the frame `image` shows. All arithmetic is f32 and unfused, one rounding per operation, in the order written; sqrt
 * and / are the correctly rounded ones; clamp01(v) = fminf(fmaxf(v, 0.0f), 1.0f), so a NaN becomes 0. With R = (float)max_radius:
 *   Half velocity of pixel (x, y), index p = y*width + x, record r:
 *     dx = ((float)x + 0.5f) - r.prev_x,  dy = ((float)y + 0.5f) - r.prev_y,  s = 0.5f * shutter
 *     hx = dx * s,  hy = dy * s,  len = sqrt(hx*hx + hy*hy)
 *     hx = hy = len = 0 when PYR_MOTION_IN_FRONT is clear or prev_x, prev_y or len is not finite; otherwise, if len > R:
 *     k = R / len, hx = hx * k, hy = hy * k, len = R.
 *     The blur is centred on the frame: taps span X - n .. X + n, for linear motion the exposure [t - shutter/2, t + shutter/2].
 *   Depth of a pixel: z = r.depth with PYR_MOTION_HIT, else FLT_MAX (a miss lies behind everything; nothing forms inf - inf).
 *   Tile maximum: tiles are max_radius x max_radius pixels, tile (tx, ty) = (x / max_radius, y / max_radius), index ty*tiles_x + tx,
 *     partial at the right and bottom edges. A tile's maximum is the (hx, hy, len) of its pixel of largest len; of equal ones,
 *     the one of smallest p.
 *   Neighbour maximum (nx, ny, ln) of a tile: the tile maximum of largest len among the up to nine tiles of its 3 x 3 block that
 *     lie inside the tile grid; of equal ones, the one of smallest tile index.
 *   Gather, per pixel X = (x, y) with its tile's neighbour maximum, colour C_X = image[p], (lenX, zX) from above:
 *     If ln < 0.5f, or one of C_X's three floats is not finite: out[p] = image[p], bit for bit. Otherwise
 *     lX = fmaxf(lenX, 0.5f),  w0 = 1.0f / lX,  W = w0,  S_c = w0 * C_X.c.
 *     Jitter: k = p + seed * 0x9E3779B1u;  k ^= k >> 16;  k *= 0x7FEB352Du;  k ^= k >> 15;  k *= 0x846CA68Bu;  k ^= k >> 16  (uint32,
 *     wrapping);  j = (float)(k >> 8) * 0x1p-24f - 0.5f,  in [-0.5, 0.5).
 *     For i = 0 .. samples-1, in order:
 *       t = ((((float)i + 0.5f) + j) / (float)samples) * 2.0f - 1.0f;   ox = nx * t,  oy = ny * t
 *       ax = floorf(((float)x + 0.5f) + ox),  ay = floorf(((float)y + 0.5f) + oy);  the tap Y = (ax, ay) is skipped unless
 *       0 <= ax < (float)width and 0 <= ay < (float)height (decided on the floats, before any cast), and skipped when one of the
 *       three floats of C_Y is not finite. With (lenY, zY) of Y:
 *       dist = sqrt(ox*ox + oy*oy),  lY = fmaxf(lenY, 0.5f),  e = depth_softness * fmaxf(zX, zY)
 *       front(a, b) = clamp01(1.0f - (a - b) / e)                     -- 1 where a lies in front of b
 *       cone(d, l) = clamp01(1.0f - d / l)
 *       cyl(d, l):  lo = 0.95f * l,  hi = 1.05f * l,  u = clamp01((d - lo) / (hi - lo)),  cyl = 1.0f - (u*u) * (3.0f - 2.0f*u)
 *       w = (front(zY, zX) * cone(dist, lY) + front(zX, zY) * cone(dist, lX)) + (cyl(dist, lY) * cyl(dist, lX)) * 2.0f
 *       W = W + w,  S_c = S_c + w * C_Y.c
 *     out[p].c = S_c / W.
 * A moving pixel reads at most 1 + samples pixels, all inside the 3 x 3 block of tiles around its own. One lane owns a pixel, there
 * are no atomics, two calls write the same bytes. The records describe first hits only: shadows and reflections do not blur, a
 * sphere's rotation and lens blur are not tracked (as above), and one previous frame gives linear motion. One GPU. */
#define PYR_MOTION_BLUR_SHUTTER 0.5f
#define PYR_MOTION_BLUR_SAMPLES 15u
#define PYR_MOTION_BLUR_MAX_RADIUS 16u
#define PYR_MOTION_BLUR_DEPTH_SOFTNESS 0.02f /* relative, like PYR_REPROJECT_DEPTH_TOLERANCE */
#define PYR_MOTION_BLUR_MOST_SAMPLES 64u
#define PYR_MOTION_BLUR_MOST_RADIUS 64u
typedef struct PyrMotionBlurParams {
    float shutter;        /* the fraction of the frame interval the shutter is open: finite, in (0, 1] */
    uint32_t samples;     /* taps per pixel, 1..64 */
    uint32_t max_radius;  /* the largest half-length of a blur in pixels, and the tile edge: 1..64 */
    float depth_softness; /* finite, > 0 */
    uint32_t seed;        /* of the per-pixel jitter */
    uint32_t reserved[3]; /* 0 */
} PyrMotionBlurParams; /* 32 bytes */
/* Arguments are checked before a device is looked for: PYR_ERR_INVALID_ARGUMENT, with the argument named in pyr_last_error, for a
 * null image, motion, params or out, an empty image, a parameter out of range (a NaN is), a non-zero reserved word;
 * PYR_ERR_UNSUPPORTED for more than 2^32 - 1 pixels; only then PYR_ERR_DEVICE. HOST buffers. Blocking. */
int pyr_image_motion_blur(const float* image, const PyrMotionPixel* motion, uint32_t width, uint32_t height, const PyrMotionBlurParams* params, float* out, int device);
/* The same with every buffer resident on `device`, enqueued on `hip_stream`. The records must be 16-byte aligned and out may not
 * overlap image or motion (PYR_ERR_INVALID_ARGUMENT otherwise). Working memory -- 16 bytes a pixel and 32 a tile -- is allocated
 * and freed in stream order. */
int pyr_image_motion_blur_device(const float* image_device, const PyrMotionPixel* motion_device, uint32_t width, uint32_t height,
                                 const PyrMotionBlurParams* params, float* out_device, int device, void* hip_stream);
/* What pyr_session_linear (PYR_LINEAR_SRGB), pyr_session_motion and the blur do, composed on the session's stream and device:
 * nothing but the result crosses to the host. out = HOST, height*width*3 floats. The session's film is not touched, and further
 * passes may follow. Blocking. */
int pyr_session_motion_blurred(PyrSession* session, const PyrCamera* previous_camera, const PyrDevelopParams* develop_params,
                               const PyrMotionBlurParams* blur_params, float* out);

/* ---------------------------------------------------------------- temporal resolve ----
 * pyr_image_reproject starts a pixel's mean again only when its surface was hidden a frame ago: it watches shape and depth. Light
 * that changes on a surface that stays -- a shadow that moves off a floor, a lamp that changes colour, what a mirror shows -- is kept
 * for up to max_history frames and trails behind everything that moves. The resolve fetches the history exactly as the
 * reprojection does, then clips it to the box that the neighbourhood of `current` spans (Karis, "High Quality Temporal
 * Supersampling", SIGGRAPH 2014 course; the variance box of Salvi, "An Excursion in Temporal Supersampling", GDC 2016) and lets a
 * pixel whose history had to be clipped forget faster. It needs no scene.
 *   `current`, `history`, `out`: width*height*3 f32 in linear light; `motion`, `history_motion`: the records; `history_count`,
 * `count_out`: one f32 a pixel; the three history buffers are all NULL (a first frame) or all given. `noise`: optional (NULL =
 * absent), width*height*3 f32, the error_out of pyr_image_denoise for the frame `current` shows, read as fabsf(noise): it widens the
 * box by the noise the frame is known to have left. `clip_out`: optional (NULL = not wanted), one f32 a pixel.
 *   All arithmetic is f32 and unfused, one rounding per operation, in the order written; sqrt and / are the correctly rounded ones;
 * fminf and fmaxf drop a NaN operand as C's do. Per pixel p with record r:
 *   1. Usable. A pixel q is usable iff the three floats of current[q] are finite and, when `noise` is given, those of noise[q] are
 *      too. If p is not usable: out = current bit for bit, count_out = 1, clip_out = 0.
 *   2. Moments. q runs over the (2*radius+1)^2 neighbourhood of p in raster order, dy outer, dx inner; pixels outside the image or
 *      not usable are skipped; k is the number kept, as a float (p itself always is). Per channel c, each sum from 0.0f:
 *        mean_c = (sum of current_c(q)) / k
 *        in a second walk in the same order  d = current_c(q) - mean_c,  var_c = (sum of d*d) / k,  sigma_c = sqrt(var_c)
 *        nbar_c = (sum of fabsf(noise_c(q))) / k, or 0.0f without a noise image
 *      Two walks, not E[x^2] - E[x]^2: a lamp's pixels are in the hundreds, and the difference of squares loses there what the
 *      clip needs.
 *   3. History fetch: that of pyr_image_reproject, word for word -- the four taps, what makes a tap count, Wt, Hc, N. Where that
 *      rule says "no history": out = current, count_out = 1, clip_out = 0. Otherwise H_c = Hc / Wt, n = fminf(N / Wt, max_history).
 *   4. Clip.  e_c = gamma * sigma_c + noise_scale * nbar_c,  lo_c = mean_c - e_c,  hi_c = mean_c + e_c
 *        H'_c = fminf(fmaxf(H_c, lo_c), hi_c)
 *        q_c = fabsf(H_c - H'_c) / fmaxf(e_c, 1e-30f)              -- how far outside the box, in half-widths of the box
 *        r = fminf(fmaxf(fmaxf(q_0, q_1), q_2), 1e30f)
 *   5. Forget and blend.  n2 = n / (1.0f + response * r)
 *        out_c = H'_c + (current_c - H'_c) / (n2 + 1.0f),  count_out = n2 + 1.0f,  clip_out = r
 * A pixel whose history already lies in the box has r = 0, n2 = n and H' = H: it is, bit for bit, what pyr_image_reproject writes
 * (a zero may differ in sign: fmaxf(-0, +0) is either). One lane owns a pixel, there are no atomics, two calls write the same
 * bytes. The box is per channel in linear RGB and clamps, it does not clip towards the centre; the fetch is bilinear; no variance
 * is carried across frames. One GPU. */
#define PYR_TEMPORAL_RADIUS 1u
#define PYR_TEMPORAL_GAMMA 1.0f
#define PYR_TEMPORAL_NOISE_SCALE 1.0f
#define PYR_TEMPORAL_RESPONSE 1.0f
#define PYR_TEMPORAL_MOST_RADIUS 3u
typedef struct PyrTemporalParams {
    float depth_tolerance; /* >= 0, finite: as PyrReprojectParams; default PYR_REPROJECT_DEPTH_TOLERANCE */
    float max_history;     /* >= 1, finite: as PyrReprojectParams; default PYR_REPROJECT_MAX_HISTORY */
    uint32_t radius;       /* 1..PYR_TEMPORAL_MOST_RADIUS: the neighbourhood is (2*radius+1)^2 pixels */
    float gamma;           /* >= 0, finite: the half-width of the box in standard deviations */
    float noise_scale;     /* >= 0, finite: how far the noise image widens the box */
    float response;        /* >= 0, finite: how fast a clipped pixel forgets; 0 = the reprojection's count */
    uint32_t reserved[2];  /* 0 */
} PyrTemporalParams; /* 32 bytes */
/* Arguments are checked before a device is looked for: PYR_ERR_INVALID_ARGUMENT, with the argument named in pyr_last_error, for a
 * null current, motion, params, out or count_out, history buffers of which some but not all are NULL, an empty image, a parameter
 * out of range (a NaN is), a non-zero reserved word; PYR_ERR_UNSUPPORTED for more than 2^32 - 1 pixels; only then PYR_ERR_DEVICE.
 * HOST buffers. Blocking. */
int pyr_image_temporal_resolve(const float* current, const PyrMotionPixel* motion, const float* noise, const float* history, const PyrMotionPixel* history_motion,
                               const float* history_count, uint32_t width, uint32_t height, const PyrTemporalParams* params, float* out, float* count_out,
                               float* clip_out, int device);
/* The same with every buffer resident on `device`, enqueued on `hip_stream`. The two record arrays must be 16-byte aligned, and no
 * output may overlap an input or another output (PYR_ERR_INVALID_ARGUMENT otherwise). */
int pyr_image_temporal_resolve_device(const float* current_device, const PyrMotionPixel* motion_device, const float* noise_device, const float* history_device,
                                      const PyrMotionPixel* history_motion_device, const float* history_count_device, uint32_t width, uint32_t height,
                                      const PyrTemporalParams* params, float* out_device, float* count_out_device, float* clip_out_device, int device,
                                      void* hip_stream);

/* ---------------------------------------------------------------- glare ----
 * Both tone curves turn a pixel of 40 and one of 4000 into the same white with the same hard edge. The glare is what a lens or an
 * eye adds: a little of every pixel's light scattered over its surroundings with a long tail, so that what is brighter than white
 * shows by the glow around it. The point spread is the normalised sum of L blurs, each twice as wide as the one before, computed
 * as a pyramid: L halvings of the source, then L doublings that add a level on the way up (the dual filtering used for bloom in
 * real-time renderers, e.g. Jimenez, "Next Generation Post Processing in Call of Duty: Advanced Warfare", SIGGRAPH 2014 course).
 * It needs no scene. `image`, `out`: width*height*3 f32 in linear light.
 *   All arithmetic is f32 and unfused, one rounding per operation, in the order written; / is the correctly rounded one;
 * clamp01(v) = fminf(fmaxf(v, 0.0f), 1.0f) as above, so a NaN becomes 0.
 *   Kept pixels. A pixel p whose three floats are not all finite is not kept: out[p] = image[p] bit for bit, and its source is 0.
 *   Source S0 of a kept pixel (R, G, B), with Y = (0.2126f*R + 0.7152f*G) + 0.0722f*B as in the statistics:
 *     threshold == 0:  S0 = image, the same bits (no multiply).
 *     otherwise:       k = clamp01((Y - threshold) / fmaxf(Y, 1e-30f)),  S0.c = image.c * k.
 *   Level sizes. w_0 = width, h_0 = height, w_{l+1} = (w_l + 1) / 2, h likewise (integer division). L = min(levels, the number of
 *     steps until a level is 1 x 1). L = 0 for a 1 x 1 image: out = image, bit for bit.
 *   Down, S_{l+1} from S_l: separable, rows first, then columns. With the values a, b, c, d of the taps at 2x-1, 2x, 2x+1, 2x+2,
 *     each tap clamped to [0, w_l - 1]:
 *       (a + d) * 0.125f + (b + c) * 0.375f
 *     The columns do the same to the row results (taps at 2y-1 .. 2y+2 clamped to [0, h_l - 1]); a row result is an f32.
 *   Up, Up(T) from level l+1 to level l: separable, rows first, then columns. With i = x >> 1:
 *       even x:  T[i] * 0.75f + T[max(i-1, 0)] * 0.25f
 *       odd x:   T[i] * 0.75f + T[min(i+1, w_{l+1}-1)] * 0.25f
 *     and the columns the same on the row results with j = y >> 1 and h_{l+1}.
 *   Weights, on the host in f32:  g_1 = 1.0f,  g_{l+1} = g_l * falloff,  G = ((g_1 + g_2) + ...) + g_L,  inv = 1.0f / G.
 *   Accumulate.  T_L = S_L * g_L;   T_l = S_l * g_l + Up(T_{l+1}) for l = L-1 .. 1;   B = Up(T_1) * inv.
 *   Compose, per kept pixel:  out.c = (image.c - strength * S0.c) + strength * B.c.
 * This is a convolution with (1 - strength) * delta + strength * PSF. Every stage's weights sum to 1, so a constant image stays
 * constant; away from the border light is moved, not made. At the border the taps are clamped, not dropped and renormalised: that
 * keeps a constant image constant and gives up conservation there -- the edge pixels count more than once, so a bright pixel at
 * the border spreads a little more light than it loses. With falloff = 1 the response to an impulse falls roughly as r^-2.
 *   One lane owns a pixel, there are no atomics, two calls write the same bytes. No streaks, stars or ghosts, no aperture-shaped or
 * wavelength-dependent point spread. One GPU.
 *   The defaults are a maintainer's choice of a plausible eye, not measured values. */
#define PYR_GLARE_STRENGTH 0.1f
#define PYR_GLARE_LEVELS 6u
#define PYR_GLARE_THRESHOLD 0.0f
#define PYR_GLARE_FALLOFF 1.0f
#define PYR_GLARE_MOST_LEVELS 12u
typedef struct PyrGlareParams {
    float strength;       /* finite, in (0, 1]: the share of the source that is spread */
    uint32_t levels;      /* 1..PYR_GLARE_MOST_LEVELS; more than the image has count as all it has */
    float threshold;      /* finite, >= 0: luminance below which a pixel spreads nothing; 0 = every kept pixel spreads */
    float falloff;        /* finite, in (0, 4]: the weight of a level over that of the level before it */
    uint32_t reserved[4]; /* 0 */
} PyrGlareParams; /* 32 bytes */
/* Arguments are checked before a device is looked for: PYR_ERR_INVALID_ARGUMENT, with the argument named in pyr_last_error, for a
 * null image, params or out, an empty image, a parameter out of range (a NaN is), a non-zero reserved word; PYR_ERR_UNSUPPORTED
 * for more than 2^32 - 1 pixels; only then PYR_ERR_DEVICE. HOST buffers. Blocking. */
int pyr_image_glare(const float* image, uint32_t width, uint32_t height, const PyrGlareParams* params, float* out, int device);
/* The same with both buffers resident on `device`, enqueued on `hip_stream`. out may not overlap image (PYR_ERR_INVALID_ARGUMENT
 * otherwise). Working memory -- levels 1..L, 16 bytes a pixel: fewer than width*height/3 + width + height + 12 pixels -- is
 * allocated and freed in stream order. */
int pyr_image_glare_device(const float* image_device, uint32_t width, uint32_t height, const PyrGlareParams* params, float* out_device, int device, void* hip_stream);
/* What pyr_session_linear (PYR_LINEAR_SRGB) and the glare do, composed on the session's stream and device: nothing but the result
 * crosses to the host. out = HOST, height*width*3 floats. The session's film is not touched, and further passes may follow.
 * Blocking. */
int pyr_session_glared(PyrSession* session, const PyrDevelopParams* develop_params, const PyrGlareParams* glare_params, float* out);

/* ------------------------------------------------------------- upsample ----
 * Rendering dominates the cost of a frame, and the first-hit feature pass is noise-free, deterministic and cheap at any size. This
 * joins the two: a joint bilateral upsampling (Kopf et al., "Joint Bilateral Upsampling", SIGGRAPH 2007) of a linear image rendered
 * at low_width x low_height to W x H with W = scale*low_width, H = scale*low_height exactly, steered by full-size normals, depths
 * and material ids so that it does not blur across an outline, and demodulated by albedo so that texture detail comes back at full
 * size although the light was sampled at a fraction of it. It needs no scene.
 *   `low`: low_width*low_height*3 f32 in linear light; `out`: W*H*3 f32. The albedo pair -- `low_albedo` at the low size, `albedo`
 * at W x H, three floats a pixel -- is optional: both given or both NULL. So is the records pair `low_pixels`, `pixels`.
 *   All arithmetic is f32 and unfused, one rounding per operation, in the order written; / is the correctly rounded one; sums start
 * from 0.0f and run in the order written; the channel loop c = 0, 1, 2 is innermost. There is no expf: every bit is pinned.
 *   Position. For the output pixel P = (X, Y):  lx = ((float)X + 0.5f) / (float)scale - 0.5f,  x0 = (int)floorf(lx);  ly, y0 alike.
 *   Taps. q = (qx, qy) = (x0 - (radius-1) + i, y0 - (radius-1) + j) for j = 0 .. 2*radius-1 (outer), i = 0 .. 2*radius-1. A tap
 *     outside the low image is skipped.  sx = fmaxf(1.0f - fabsf((float)qx - lx) / (float)radius, 0.0f),  sy alike,  sp = sy * sx.
 *     A tap with sp == 0 is skipped. The taps that are left are the taps kept. With radius 1 and neither pair this is bilinear
 *     interpolation, the edges clamped by renormalisation.
 *   Guide weight gw, with the records pair (without it gw = 1). D = 0.0f. Each term applies only when its sigma is > 0, in this
 *     order; a term g that is a NaN makes gw = 0 whatever else holds, any other sets D = fmaxf(D, g):
 *       normal:  g = (((0.0f + e_0*e_0) + e_1*e_1) + e_2*e_2) / (2.0f * (sigma_normal*sigma_normal)),  e_c = normal_c(P) - normal_c(q)
 *       depth:   m = fmaxf(fmaxf(z_P, z_q), 1e-30f),  r = (z_P - z_q) / m,  g = (r*r) / (2.0f * (sigma_depth*sigma_depth))
 *     (the denoiser's distances). t = 1.0f - D;  gw = t*t when t > 0, else 0: the support is compact, a tap further than
 *     sigma*sqrt(2) away weighs exactly 0. With PYR_UPSAMPLE_MATCH_MATERIAL gw = 0 when PyrFeaturePixel::material of q and of P
 *     differ: that keeps a lamp set flush into a ceiling (same normal, same depth, no albedo channel) out of the ceiling's pixels.
 *     w = sp * gw.
 *   Demodulation, with the albedo pair (without it v_c = low_c(q)). Per low pixel and channel:
 *       d_c(q) = 1.0f / (fmaxf(low_albedo_c(q), 0.0f) + albedo_floor)
 *     per tap:  k_c = fminf((fmaxf(albedo_c(P), 0.0f) + albedo_floor) * d_c(q), max_gain), a NaN k_c counting as max_gain;
 *     v_c = low_c(q) * k_c. The two fmaxf change nothing for an albedo that is not negative. A developed albedo can be: a saturated
 *     colour lies outside linear sRGB, and without them low_albedo_c + albedo_floor would cross 0 and the gain have no bound (a NaN
 *     albedo counts as 0). So 0 <= k_c <= max_gain always.
 *   Sums over the taps kept, in tap order:  S += sp,  B_c += sp * low_c(q)  for every one of them;  W_ += w,  A_c += w * v_c  for
 *     those with w > 0 only -- a tap of weight 0 adds nothing, so its NaN cannot leak.
 *   Output.  out_c = A_c / W_ when W_ > 0, otherwise out_c = B_c / S: the raw tent, not demodulated, so that a pixel every guide
 *     rejects never explodes. S > 0 always: the low pixel that contains P is inside and weighs more than 0.25.
 * A tap that is not finite and has positive weight makes its output pixels not finite; which pixels and which of inf, -inf and NaN
 * follows from the rule, the sign and payload bits of a NaN do not. One lane owns an output pixel, stores are plain, there are no
 * float atomics: two calls write the same bytes. Integer scales only; nothing is reused over time. One GPU.
 *   The defaults: the denoiser's sigmas; the floor and the gain are a maintainer's choice. */
#define PYR_UPSAMPLE_RADIUS 1u
#define PYR_UPSAMPLE_MOST_RADIUS 3u
#define PYR_UPSAMPLE_MOST_SCALE 8u
#define PYR_UPSAMPLE_SIGMA_NORMAL 0.1f /* = PYR_DENOISE_SIGMA_NORMAL */
#define PYR_UPSAMPLE_SIGMA_DEPTH 0.02f /* = PYR_DENOISE_SIGMA_DEPTH */
#define PYR_UPSAMPLE_ALBEDO_FLOOR 0.01f
#define PYR_UPSAMPLE_MAX_GAIN 4.0f
#define PYR_UPSAMPLE_MATCH_MATERIAL 1u
typedef struct PyrUpsampleParams {
    uint32_t radius;      /* 1..PYR_UPSAMPLE_MOST_RADIUS: 2*radius taps per axis */
    uint32_t flags;       /* PYR_UPSAMPLE_MATCH_MATERIAL or 0; other bits are refused */
    float sigma_normal;   /* <= 0 (or NaN) turns that guide off */
    float sigma_depth;    /* likewise */
    float albedo_floor;   /* > 0; read when the albedo pair is given */
    float max_gain;       /* >= 1; likewise */
    uint32_t reserved[2]; /* 0 */
} PyrUpsampleParams; /* 32 bytes */
/* Arguments are checked before a device is looked for: PYR_ERR_INVALID_ARGUMENT, with the argument named in pyr_last_error, for a
 * null low, params or out, half a pair, an empty image (low_width, low_height), a scale outside 2..PYR_UPSAMPLE_MOST_SCALE, a
 * radius outside 1..3, an unknown flag bit, with the albedo pair an albedo_floor that is not > 0 or a max_gain that is not >= 1 (a
 * NaN is neither), a non-zero reserved word; PYR_ERR_UNSUPPORTED when W*H exceeds 2^32 - 1, or W or H 2^24, up to which (float)X
 * is exact; only then PYR_ERR_DEVICE. HOST buffers. Blocking. */
int pyr_image_upsample(const float* low, const float* low_albedo, const PyrFeaturePixel* low_pixels, uint32_t low_width, uint32_t low_height, uint32_t scale,
                       const float* albedo, const PyrFeaturePixel* pixels, const PyrUpsampleParams* params, float* out, int device);
/* The same with every buffer resident on `device`, enqueued on `hip_stream`. The records are read as 16-byte vectors: a records
 * pointer that is not 16-byte aligned is PYR_ERR_INVALID_ARGUMENT, after the checks above and before the size. No working memory. */
int pyr_image_upsample_device(const float* low_device, const float* low_albedo_device, const PyrFeaturePixel* low_pixels_device, uint32_t low_width,
                              uint32_t low_height, uint32_t scale, const float* albedo_device, const PyrFeaturePixel* pixels_device, const PyrUpsampleParams* params,
                              float* out_device, int device, void* hip_stream);
/* The session's film, width x height, is the low image. On the session's stream and device: with `denoise_params` what
 * pyr_session_denoised does (PYR_SESSION_HALVES and two passes, the same refusals; `feature_params` steers that filter too), without
 * them what pyr_session_linear does in PYR_LINEAR_SRGB; with `feature_params` the feature pass at the session's size -- the one the
 * denoiser ran, when it ran -- and once more with the session's camera and a film of scale*width x scale*height, both albedo
 * films developed with `develop_params`; then the upsample, with both pairs or, without `feature_params`, with neither.
 * out = HOST, scale*height * scale*width * 3 floats. The session's films are not touched, and further passes may follow. Blocking. */
int pyr_session_upsampled(PyrSession* session, uint32_t scale, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params,
                          const PyrDenoiseParams* denoise_params, const PyrUpsampleParams* upsample_params, float* out);

/* ------------------------------------------------------------ despeckle ----
 * Every image stage above assumes noise that behaves. A path tracer's does not: dispersive glass, small lamps and mirrors give, at
 * preview sample counts, fireflies -- single pixels, in one half only, tens to thousands of times brighter than what surrounds them.
 * The cross filter reads its weights from the other half, so it cannot see one and smears it over its window; the glare gives it a
 * halo; the percentiles of the tone curve move. The two halves hold what tells a firefly from a highlight: a one-pixel lamp or
 * glint is bright in both independent halves, a firefly in one. This clamps the second kind and keeps the first. It needs no scene.
 *   `a`, `b`, `a_out`, `b_out`, `removed_out`: width*height*3 f32 in linear light. `b` and `b_out` are given together or both NULL;
 * without them the filter works on one image, the agreement test below is dropped, and more is clamped along edges.
 *   All arithmetic is f32 and unfused, one rounding per operation, in the order written; / is the correctly rounded one. "Finite"
 * means neither an infinity nor a NaN.
 *   Luminance, of every pixel of every given half:  Y = ((0.2126f*R + 0.7152f*G) + 0.0722f*B) + 0.0f  -- the statistics' expression;
 *     the + 0.0f turns a -0 into +0, so that no -0 enters an ordering.
 *   Sample set N(p): Y_H(q) for each given half H and each q of the (2*radius+1)^2 window around p clipped to the image, q = p
 *     excluded (in both halves), finite values only. n = the number of them, at most 48. With n < PYR_DESPECKLE_LEAST_SAMPLES both
 *     halves keep their bits at p.
 *   Median and spread.  m = the lower median of N(p): element (n-1)/2 (integer division) of its ascending order.
 *     s = the lower median, the same element, of fabsf(Y_i - m) over the same set.
 *     spread = fmaxf(fmaxf(s * 1.4826f, relative * m), floor);   limit = m + k * spread.
 *     Medians are selections, not sums: whatever algorithm selects, the bits are the same.
 *   The firefly test. Half H holds a firefly at p when Y_H(p) is finite and Y_H(p) > limit and -- with the other half given -- it
 *     is not the case that the other half's Y(p) is finite and > limit. The last clause keeps lamps, glints and the bright side of
 *     an edge: what both halves saw.
 *   The clamp.  g = limit / Y_H(p);  out_H(p).c = in_H(p).c * g: the hue is kept, the luminance lands on the limit. Every other
 *     pixel of either half keeps its bits, the pixels that are not finite among them. (limit > 0 whenever m >= 0. A neighbourhood
 *     whose median luminance is negative -- out-of-gamut colours throughout -- can make limit <= 0; g is then what the division gives.)
 *   Reports, both optional.  d_H(p).c = in_H(p).c - out_H(p).c where H was clamped at p, 0.0f elsewhere.
 *     removed_out(p).c = (d_a + d_b) * 0.5f with b, d_a without: the energy the mean of the halves lost, and where. For finite
 *     pixels this is ((a - a_out) + (b - b_out)) * 0.5f bit for bit; at a pixel that is not finite it is 0.0f, not the NaN that
 *     inf - inf would make, whose sign two IEEE machines need not agree on.
 *     counts_out[0], counts_out[1]: the pixels clamped in a and in b (0 without b), summed by integer atomics.
 * One lane owns a pixel, stores are plain, there is no float reduction: two calls write the same bytes. Outputs may not overlap
 * inputs or each other: the rule reads neighbourhoods. No spectral form, no guides: the agreement of the halves does their job.
 *   The defaults k = 6, relative = 0.1 come from a synthetic prototype (log-normal noise, planted outliers), not from renders. */
#define PYR_DESPECKLE_RADIUS 2u
#define PYR_DESPECKLE_MOST_RADIUS 2u
#define PYR_DESPECKLE_K 6.0f
#define PYR_DESPECKLE_RELATIVE 0.1f
#define PYR_DESPECKLE_FLOOR 1e-4f
#define PYR_DESPECKLE_LEAST_SAMPLES 5u
typedef struct PyrDespeckleParams {
    uint32_t radius;      /* 1..PYR_DESPECKLE_MOST_RADIUS: the window is (2*radius+1)^2 pixels */
    float k;              /* finite, > 0: spreads above the median at which a pixel is a firefly */
    float relative;       /* finite, >= 0: the spread is at least this share of the median */
    float floor;          /* finite, > 0: and at least this much, which serves a black neighbourhood */
    uint32_t flags;       /* none defined: any bit is refused */
    uint32_t reserved[3]; /* 0 */
} PyrDespeckleParams; /* 32 bytes */
/* Arguments are checked before a device is looked for, in this order: PYR_ERR_INVALID_ARGUMENT, with the argument named in
 * pyr_last_error, for a null a, params or a_out; for b without b_out or b_out without b; for an empty image (width, height);
 * PYR_ERR_UNSUPPORTED for more than 2^32 - 1 pixels; PYR_ERR_INVALID_ARGUMENT again for a radius outside 1..2, a k or floor that is
 * not finite and > 0, a relative that is not finite and >= 0, any flag bit, a non-zero reserved word, and for an output that
 * overlaps an input or another output (the same pointer given twice does); only then PYR_ERR_DEVICE. counts_out: two uint32_t.
 * HOST buffers. Blocking. */
int pyr_image_despeckle(const float* a, const float* b, uint32_t width, uint32_t height, const PyrDespeckleParams* params, float* a_out, float* b_out,
                        float* removed_out, uint32_t* counts_out, int device);
/* The same with every buffer resident on `device`, enqueued on `hip_stream`. No output may overlap an input or another output
 * (PYR_ERR_INVALID_ARGUMENT otherwise): a workgroup reads the neighbourhood of its tile while another writes. No working memory. */
int pyr_image_despeckle_device(const float* a_device, const float* b_device, uint32_t width, uint32_t height, const PyrDespeckleParams* params, float* a_out_device,
                               float* b_out_device, float* removed_out_device, uint32_t* counts_out_device, int device, void* hip_stream);
/* On the session's stream and device (PYR_SESSION_HALVES and two passes, as pyr_session_denoised): half film A alone and half film
 * B alone developed to linear sRGB, despeckled, and then, with `denoise_params`, cross filtered as pyr_session_denoised filters
 * the raw halves (`feature_params`, optional, steers that filter and is not read without it); without `denoise_params`
 * out = (a' + b') * 0.5f and error_out = fabsf(a' - b') * 0.5f of the cleaned halves a', b'. out = HOST, height*width*3 floats;
 * error_out and removed_out likewise and optional; counts_out: two uint32_t, optional. The session's films are not touched, and
 * further passes may follow. Blocking. */
int pyr_session_despeckled(PyrSession* session, const PyrDevelopParams* develop_params, const PyrDespeckleParams* despeckle_params,
                           const PyrFeatureParams* feature_params, const PyrDenoiseParams* denoise_params, float* out, float* error_out, float* removed_out,
                           uint32_t* counts_out);

/* ------------------------------------------------------------ lens blur over the feature records ----
 * The feature pass is a pinhole pass, and every image stage above is steered by it: a camera with aperture > 0 renders a blur
 * whose guides are sharp. As with motion, the lens goes back in as a post filter: render the frame with aperture 0, run the
 * guide-driven filters while image and guides agree, then spread every pixel over its circle of confusion, read from the depth of
 * its record. It needs no scene. `image`, `out`: width*height*3 f32 in linear light; `pixels`: the PyrFeaturePixel records of the
 * same camera at the same size. All arithmetic is f32 and unfused, one rounding per operation, in the order written; sqrt and / are
 * the correctly rounded ones; clamp01(v) = fminf(fmaxf(v, 0.0f), 1.0f), so a NaN becomes 0; fminf and fmaxf return the other
 * operand of a NaN. "Finite" means neither an infinity nor a NaN. PI_F = 3.14159265f (0x40490FDB).
 *   The lens is the disc of radius sqrt(aperture) (cameras.rs:84). A point at axial depth z is spread on the focus plane over the
 *   radius sqrt(aperture)*|1 - f/z|, and one unit of the focus plane is view_plane/f * max(W,H)/2 pixels (cameras.rs:57-68, 78-81):
 *     m = (float)max(width, height) * 0.5f,  A = (sqrt(aperture) * (view_plane / focus_distance)) * m,  R = (float)max_radius.
 *   Circle of confusion of pixel (x, y), index p = y*width + x, record r. The record is a miss when r.coverage == 0, or r.depth is
 *   not finite, or r.depth <= 0. The pixel centre's view-plane coordinates are those of Camera::to_view_area (cameras.rs:57-68):
 *     px = ((float)x + -((float)width * 0.5f)) / m + (1.0f / m) * 0.5f,   py likewise from y and height
 *     t = (px*px + py*py) / (view_plane*view_plane)
 *     z = r.depth / sqrt(1.0f + t)                                     -- r.depth runs along the ray, z along the axis
 *     c = fminf(A * fabsf(1.0f - focus_distance / z), R)
 *   For a miss z = FLT_MAX and c = fminf(A, R): the sky lies at infinity. For every pixel
 *     inv = 1.0f / fmaxf(PI_F * ((c + 0.5f)*(c + 0.5f)), 1.0f)       -- one over the area of its disc, at most 1.
 *   (Where focus_distance / z overflows -- a depth below focus_distance / FLT_MAX -- A * inf is inf, or NaN with A = 0, and c = R.)
 *   Gather for pixel p with colour C_p = image[p] and (c_p, inv_p, z_p) from above. W_f = W_b = 0.0f, S_f = S_b = (0, 0, 0). The
 *   window is the (2*max_radius+1)^2 offsets (ox, oy), oy outer from -max_radius, ox inner from -max_radius, p itself included. A
 *   tap q = (x + ox, y + oy) is skipped when it lies outside the image or one of the three floats of C_q is not finite. Otherwise
 *     d = sqrt((float)(ox*ox + oy*oy))
 *     front = (z_p - z_q) > depth_tolerance * z_p                    -- q lies in front of p by more than the tolerance
 *     front:      c_e = c_q,  inv_e = inv_q                          -- a front tap spreads by its own circle
 *     otherwise:  c_e = fminf(c_q, c_p),  inv_e = inv_q when c_q < c_p, else inv_p
 *                                                                    -- seen only through the smaller circle: a blurred
 *                                                                       background does not bleed over a sharp foreground
 *     w = clamp01((c_e - d) + 1.0f) * inv_e
 *   A tap with w == 0 adds nothing. A front tap adds W_f = W_f + w, S_f.c = S_f.c + w * C_q.c; any other tap the same to W_b, S_b.
 *   p itself always lands in W_b with w = inv_p > 0.
 *   Result. out[p] = image[p], bit for bit, if one of C_p's three floats is not finite, or if no tap but p itself had w > 0: with
 *   aperture == 0 the filter is the identity, and what is in focus and out of every neighbour's reach keeps its bits. Otherwise
 *     B.c = S_b.c / W_b;   with W_f == 0: out[p].c = B.c;   else a = fminf(W_f, 1.0f),  F.c = S_f.c / W_f,
 *     out[p].c = a * F.c + (1.0f - a) * B.c
 *   W_f is the share of the pixel that the foreground's blur covers: a pixel wholly behind a blurred foreground shows the foreground.
 * No tap with d >= c + 1 weighs, and c <= max_radius: a pixel reads only its window. One lane owns a pixel, there are no atomics,
 * two calls write the same bytes. The limits: one layer is known per pixel, so what a wide lens sees round an edge is not
 * recovered; c is clamped to max_radius; only first hits are refocused -- a mirror's image blurs at the mirror's depth, as do
 * shadows and what glass shows. One GPU. */
#define PYR_LENS_BLUR_MAX_RADIUS 8u
#define PYR_LENS_BLUR_MOST_RADIUS 16u
typedef struct PyrLensBlurParams {
    float focus_distance;  /* PyrCamera::focus_distance: finite, > 0 */
    float aperture;        /* PyrCamera::aperture: finite, >= 0; 0 is the identity */
    float view_plane;      /* PyrCamera::view_plane: finite, > 0 */
    uint32_t max_radius;   /* the largest circle of confusion in pixels, and the window's half side: 1..PYR_LENS_BLUR_MOST_RADIUS */
    float depth_tolerance; /* relative: finite, in [0, 1); default PYR_REPROJECT_DEPTH_TOLERANCE */
    uint32_t reserved[3];  /* 0 */
} PyrLensBlurParams; /* 32 bytes */
/* Arguments are checked before a device is looked for: PYR_ERR_INVALID_ARGUMENT, with the argument named in pyr_last_error, for a
 * null image, pixels, params or out, a parameter out of range (a NaN is), a non-zero reserved word, an empty image;
 * PYR_ERR_UNSUPPORTED for more than 2^32 - 1 pixels; only then PYR_ERR_DEVICE. HOST buffers. Blocking. */
int pyr_image_lens_blur(const float* image, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height, const PyrLensBlurParams* params, float* out, int device);
/* The same with every buffer resident on `device`, enqueued on `hip_stream` without synchronising. The records must be 16-byte
 * aligned and out may not overlap image or pixels (PYR_ERR_INVALID_ARGUMENT otherwise, after the checks above and before the
 * device). No working memory. */
int pyr_image_lens_blur_device(const float* image_device, const PyrFeaturePixel* pixels_device, uint32_t width, uint32_t height, const PyrLensBlurParams* params,
                               float* out_device, int device, void* hip_stream);
/* What pyr_session_linear (PYR_LINEAR_SRGB), the records of pyr_session_features (`feature_params`; no albedo is made) and the blur
 * do, composed on the session's stream and device: nothing but the result crosses to the host. The lens is `blur_params`', not the
 * session camera's: a session rendered with aperture 0 is the intended input. out = HOST, height*width*3 floats. The session's
 * film is not touched, and further passes may follow. Blocking. */
int pyr_session_lens_blurred(PyrSession* session, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params,
                             const PyrLensBlurParams* blur_params, float* out);

#ifdef __cplusplus
}
#endif

#endif /* PYRITE_GPU_H */
