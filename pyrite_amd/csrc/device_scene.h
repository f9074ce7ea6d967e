// device_scene.h -- layout of the frozen scene in HBM, shared by the host packer (scene_pack.cpp), the uploader (scene_create.cpp) and the kernels.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/pyrite_gpu.h"

namespace pyr {

// One primitive in BVH leaf order, 48 bytes = three float4 (one dwordx4 load each):
//   triangle: a = (v1.xyz, shape), b = (edge1.xyz, 0), c = (edge2.xyz, 0)   [edges as shapes/mod.rs:44-45]
//   sphere:   a = (centre.xyz, shape), b = (radius, 0, 0, 0), c = 0
// `shape` = (PyrShapeKind << 30) | index, stored as float bits.
struct DevPrim {
    float a[4], b[4], c[4];
};

// Two triangles of one leaf of the WIDE tree, component by component, 80 bytes = five float4:
//   (v1.x[2], v1.y[2]) (v1.z[2], shape[2]) (e1.x[2], e1.y[2]) (e1.z[2], e2.x[2]) (e2.y[2], e2.z[2])
// so that a (triangle A, triangle B) pair of every component sits in an aligned register pair and both Moeller-Trumbore
// tests run in packed-f32 instructions. A leaf of n triangles owns ceil(n / 2) consecutive records; the odd one out is paired
// with an all-zero triangle (det = 0: never hit) whose shape is PYR_HIT_NONE. Only built when every primitive in the tree is
// a triangle; the wide tree's leaf codes then count in these records: -1 - (first_pair << 3 | triangles left).
struct DevPrimPair {
    float q[5][4];
};

// Shading record of a triangle, indexed by ORIGINAL triangle index, 48 bytes:
//   (n1.xyz, material), (n2.xyz, 0), (n3.xyz, 0).
struct DevTriShade {
    float n1[4], n2[4], n3[4];
};

// Texture-space record of a triangle (only uploaded for scenes that run the program interpreter), 80 bytes:
//   uv = (t1.xy, t2.xy), (t3.xy, 0, 0); frames = Vertex.normal.from_space of v1, v2, v3 as (s, x, y, z).
struct DevTriTex {
    float uv12[4], uv3[4], f1[4], f2[4], f3[4];
};

struct DevTexture {
    uint32_t channels; // 4 (LinSrgba) or 1 (LinLuma)
    uint32_t width, height;
    uint32_t reserved;
    unsigned long long offset; // floats into DevScene::texture_data
};

// Lamp with everything Lamp::sample (lamp.rs:23-82) touches pre-gathered.
struct DevLamp {
    uint32_t kind, shape_kind, shape_index, color_program;
    float v[3]; // direction / position / sphere centre
    float width; // directional: cos half angle; sphere: radius
    float p1[3], p2[3], p3[3]; // triangle lamp vertices
    float n1[3], n2[3], n3[3]; // triangle lamp vertex normals
    float area;                // Shape::surface_area
    uint32_t material;
    float t1[2], t2[2], t3[2]; // triangle lamp: vertex texture coordinates; sphere lamp: t1 = texture_scale
};

enum FastProgram : uint32_t {
    FAST_NONE = 0,         // run the interpreter
    FAST_SPECTRUM = 1,     // [SpectrumValue(wavelength)]
    FAST_SPECTRUM_MUL = 2, // [SpectrumValue(wavelength), NumberValue(c), Binary Mul]  == spectrum * c
    FAST_MUL_SPECTRUM = 3  // [NumberValue(c), SpectrumValue(wavelength), Binary Mul]  == c * spectrum
};

// How a colour program gets onto the spectral tape (kernels.hip "Spectral tape"; round 4: scenes WITH interpreter programs):
//   DIRECT     a constant or a fast shape: the record names it, the replay looks its value up per wavelength;
//   HIT_VALUE  no instruction depends on the wavelength (diamonds.lua's `mix(0, 0.2, fresnel(1.1))`): the interpreter runs it ONCE
//              per hit, where the path is shaded, and the value is folded into the record's factor;
//   HIT_RGB    everything but a closing RgbSpectrumValue(wavelength, rgb) is independent of the wavelength (a colour texture, an
//              rgb() expression): the interpreter evaluates the rgb register once per hit, the record carries its three components
//              and the replay forms rgb . RGB_basis(wavelength) per wavelength, the very sum execution_context.rs:140-152 forms;
//   LAMBDA     a function of the wavelength alone made of numbers only (`blackbody(4000) * 3`, a product or mix of spectra): like a
//              fast shape it gets a value slot -- the replay evaluates it once per item with a small number-only interpreter
//              (kernels.hip lambda_eval) -- and the record names it;
//   PRODUCT    the program's value is a chain of products ((l * h1) * h2) ... with ONE factor l that depends on the wavelength alone in
//              LAMBDA's sense and up to three factors that depend on the hit alone (a mono texture times a spectrum times a number: the
//              textured lamps of the fuzz scenes and of the generated textures scene, a tinted mask): scene_pack.cpp splits it into two programs
//              of its own instructions -- the hit side (HIT_VALUE) and the wavelength side (DIRECT or LAMBDA, with a value slot) -- the
//              interpreter runs the hit side once per hit, and records carry h1 to the slot's value, h2 ... to that product and the
//              contribution's factor to the result: the products the interpreter and `contribute` form, in their order;
//   NONE       needs an interpreter run per hit AND wavelength (a mix of spectra by a fresnel term): a
//              scene with such a COLOUR program keeps the online form of round 3 (Walker::contribute_pending).
enum TapeForm : uint32_t { TAPE_FORM_DIRECT = 0, TAPE_FORM_HIT_VALUE = 1, TAPE_FORM_HIT_RGB = 2, TAPE_FORM_NONE = 3, TAPE_FORM_LAMBDA = 4, TAPE_FORM_PRODUCT = 5 };

struct DevProgram {
    uint32_t kind; // PyrProgramKind
    float constant;
    uint32_t first_instr, num_instrs;
    uint32_t output_kind, output_reg;
    uint32_t fast;            // FastProgram
    uint32_t fast_spectrum;   // spectrum id of the fast forms
    float fast_scale;         // c of the fast forms
    uint32_t reads_wavelength; // some executed operand is Input(Wavelength): ProbabilityInput::wavelength_used
    uint32_t tape_form;        // TapeForm
    // HIT_RGB: the rgb register the closing RgbSpectrumValue reads. PRODUCT (one word, so that the record stays twelve: three more were 8 % of
    // the example scenes' throughput): bits 0-7 / 8-15 the two programs scene_pack.cpp made of this one's instructions, the hit side and the
    // wavelength side; bits 16-19 the number of hit-side factors (1-3), bits 20-23, 24-27, 28-31 their number registers, innermost product first
    uint32_t tape_rgb_reg;
};

struct DevScene {
    const float* nodes;  // Node64[], 16 floats each
    const float* wide_nodes; // Node128[], 32 floats each, or nullptr: the tree the resumable traversal walks on big scenes
    uint32_t wide_stack_depth; // stack entries that tree can need
    const float* pair_prims;      // DevPrimPair[], or nullptr
    const float* wide_pair_nodes; // the wide tree once more with leaf codes that count in DevPrimPair records (the stage-scheduled render walks this copy; the ray-batch kernels keep the one-primitive records: they are bound by bytes through L1, and a pair is 80 B where a lone triangle is 48)
    const float* prims;  // DevPrim[], 12 floats each
    const float* tri_shade; // DevTriShade[]
    const float* spheres;   // [n][4] centre, radius (original order)
    const uint32_t* sphere_material;
    const float* planes;    // [n][8]
    const uint32_t* plane_material;
    const DevLamp* lamps;
    const PyrMaterial* materials;
    const PyrComponent* components;
    const DevProgram* programs;
    const PyrInstr* instrs;
    const PyrSpectrum* spectra;
    const float* spectrum_data;
    const float* rgb_basis;
    uint32_t num_planes, num_lamps;
    uint32_t rgb_count;
    float rgb_min, rgb_max;
    uint32_t sky_program;
    uint32_t stack_depth; // LDS stack entries per lane = BVH max depth
    uint32_t needs_interpreter; // some program is neither a constant nor a fast shape
    uint32_t num_nodes, num_prims;
    uint32_t num_spectra, num_spectrum_floats;
    uint32_t num_programs;
    uint32_t num_materials, num_components;
    uint32_t lds_table_floats; // > 0: spectra, materials, components, programs and lamps are staged into LDS (this many floats in all)
    // texture space (interpreter builds only)
    const float* tri_tex;          // DevTriTex[] by original triangle index, or nullptr
    const float* sphere_tex_scale; // [n][2]
    const float* plane_frames;     // [n][4] quaternion (s, x, y, z)
    const DevTexture* textures;
    const float* texture_data;
    uint32_t uses_textures; // some program holds a texture opcode or some material a normal map
    // some emissive component's probability program reads the wavelength: a light sample of such a material is added for the hero
    // wavelength only (algorithm.rs:78), i.e. the spectral tape can hold hero-only records. No BASELINE scene has one.
    uint32_t hero_only_records;
    // needs_interpreter != 0 and every colour program (components, lamps, sky) has a tape form: the stage scheduler records a tape
    // for this scene too and the interpreter runs once per hit instead of once per hit and wavelength
    uint32_t hit_tape;
    uint32_t rgb_records; // some colour program is HIT_RGB: its contributions are four records (three coefficients + the factor)
    uint32_t product_records; // some colour program is PRODUCT: the scene runs the PRODUCT builds of the hit-tape kernels
    uint32_t micro_records; // some colour program is HIT_RGB or PRODUCT: the replay reads bits 12-14 of a record (kernels.hip TAPE_RGB_*)
    // Boxes a shadow ray may skip lie beyond limit * shadow_margin (+ 1e-3), limit = the blocking limit (a squared distance): 1.001
    // covers the ulps between a box's entry distance and a triangle's hit distance; scenes with spheres take 1.01 -- collision's
    // sphere routine loses every digit of l.l - tca^2 for a ray that passes at a thousand radii or more and then reports hits up to a
    // radius NEARER than the sphere's own box, which the reference, walking with closest = inf, still counts as blockers.
    float shadow_margin;
    uint32_t tape_value_rows; // LDS value rows of the eager replay (above): 8, or as many as the scene's spectrum-reading programs need, up to 16; scenes without interpreter programs: tape_pair_build_rows (below)
};

// Value rows of the eager replay (kernels.hip replay_tapes): rows of BLOCK floats in LDS, one per spectrum-reading program -- its value at the
// replay item's wavelength, looked up once per item -- and one that holds 1.0 (row 7: what the records of constants and plain factors name).
// Eight rows serve every BASELINE scene (four programs); a scene with more such programs than the seven rows in front of the 1.0 gets more
// rows behind it, up to the sixteen a record's 4-bit slot field can name (DevScene::tape_value_rows): slot s lives in row s, or s + 1 from
// the seventh on; the three rows of the RGB basis stay together. (C3 with six more spectra, past the rows: 573 -> 508 Msamples/s looking
// values up record by record -- tools/bench_many_spectra.py.)
constexpr uint32_t kTapeValueRows = 8, kTapeOneRow = kTapeValueRows - 1, kTapeMaxValueRows = 16;
constexpr uint32_t tape_row(uint32_t slot) { return slot + (slot >= kTapeOneRow ? 1u : 0u); }
constexpr uint32_t tape_rgb_row(uint32_t n_spectral) { return n_spectral + 3u <= kTapeOneRow ? n_spectral : (n_spectral >= kTapeOneRow ? n_spectral + 1u : kTapeValueRows); }
constexpr uint32_t tape_rows_needed(uint32_t n_spectral, bool rgb) {
    return (rgb ? tape_rgb_row(n_spectral) + 3u : (n_spectral == 0u ? 0u : tape_row(n_spectral - 1u) + 1u)) > kTapeValueRows
               ? (rgb ? tape_rgb_row(n_spectral) + 3u : tape_row(n_spectral - 1u) + 1u)
               : kTapeValueRows;
}

// The stage scheduler's builds without interpreter programs replay a path's tape for TWO wavelengths per lane (kernels.hip replay_tapes:
// an item is a path and the halves k and k + (S + 1) / 2 of its wavelengths), in packed f32. Each value row then has a twin for the
// second half right behind it, one ds_read2st64_b32 apart: the rows come in pairs, slot 0 in pair 0, 1.0 in pair 1, slot s >= 1 in pair
// s + 1, and a record names twice its pair (up to 30: five bits of the word; bits 12-13 are the interpreter builds' alone). The pairs
// are packed -- DevScene::tape_value_rows is 2 (n + 1) rows for n spectrum-reading programs there, 10 on C3 -- because the render pays
// for every KB of LDS with a level of its traversal stack (C3: 660 Msamples/s at 14 levels, 635 at 12, profiles/r27_replay_pairs.txt).
// For the same reason these builds have no row S and let the rows start at S - 1: that row of the wavelengths only holds a draw between
// two statements of a sample's start (the hero moves to a register), and pair 0 is rewritten by every replay pass before it is read; the
// lane lists of the replay are BLOCK bytes behind the prepared programs instead of a row.
// Pairs take 2 (n + 1) rows where the layout above takes 8 (n <= 7) or n + 1, so a scene is replayed in pairs only where that costs no
// KB the layout above would not take: up to four spectrum-reading programs (tape_pairs_pay; the replay's gain is about two stack levels'
// worth). With more, these builds replay one wavelength per lane as the interpreter builds do, over single rows packed the same way
// (slots 0 and 1 in rows 0 and 1, 1.0 in row 2 -- the word a record of 1.0 carries is 2 in both forms --, slot s >= 2 in row s + 1:
// n + 1 rows, never more than the layout above). -DPYR_REPLAY_PAIRS=0 builds have the layout above throughout (A/B).
#ifndef PYR_REPLAY_PAIRS
#define PYR_REPLAY_PAIRS 1
#endif
constexpr bool tape_pairs(bool interpreter) { return PYR_REPLAY_PAIRS != 0 && !interpreter; }
constexpr uint32_t kTapeOnePair = 1, kTapeMaxPairRows = 2u * kTapeMaxValueRows, kTapePackedOneRow = 2u * kTapeOnePair;
constexpr uint32_t tape_pair(uint32_t slot) { return slot + (slot >= kTapeOnePair ? 1u : 0u); }
constexpr uint32_t tape_pair_rows(uint32_t n_spectral) { return 2u * (n_spectral + 1u); }
constexpr uint32_t tape_packed_row(uint32_t slot) { return slot + (slot >= kTapePackedOneRow ? 1u : 0u); }
constexpr uint32_t tape_packed_rows(uint32_t n_spectral) { return n_spectral < kTapePackedOneRow ? kTapePackedOneRow + 1u : n_spectral + 1u; }
constexpr bool tape_pairs_pay(uint32_t n_spectral) { return 2u * n_spectral <= tape_rows_needed(n_spectral, false); }
// (the kernel counts the programs itself and may find fewer than the host: it pairs when pairs pay AND the rows the host reserved hold them)
constexpr bool tape_replays_pairs(uint32_t n_spectral, uint32_t value_rows) { return tape_pairs_pay(n_spectral) && tape_pair_rows(n_spectral) <= value_rows; }
// the value rows of a scene with n spectrum-reading programs in these builds (too many to fit: the replay looks values up record by
// record, and row S - 1, which a sample's start draws into, is the only one: it must not be the traversal stack's)
constexpr uint32_t tape_pair_build_rows(uint32_t n_spectral) {
    return tape_pairs_pay(n_spectral) ? tape_pair_rows(n_spectral) : (tape_packed_rows(n_spectral) <= kTapeMaxValueRows ? tape_packed_rows(n_spectral) : 1u);
}
// LDS rows of a tape build in front of the traversal stack: the wavelengths, the lane lists' row (not with pairs) and the value rows;
// and where the value rows start.
constexpr uint32_t tape_first_value_row(uint32_t spectrum_samples, bool interpreter) { return tape_pairs(interpreter) ? spectrum_samples - 1u : spectrum_samples + 1u; }
constexpr uint32_t tape_spectral_rows(uint32_t spectrum_samples, uint32_t value_rows, bool interpreter) { return tape_first_value_row(spectrum_samples, interpreter) + value_rows; }
constexpr uint32_t tape_lane_list_bytes(bool interpreter) { return tape_pairs(interpreter) ? 256u : 0u; } // BLOCK lane numbers

constexpr uint32_t kMaxStackDepth = 64; // >= kMaxBvhDepth (bvh.h) and >= the wide tree's stack need (else the binary tree is walked)

// Everything one render launch needs besides the scene.
struct RenderLaunch {
    PyrCamera camera;
    PyrFilmDesc film;
    uint32_t bounces, light_samples, spectrum_samples, tile_size, pixel_samples;
    uint32_t tiles_x, tiles_y;
    // The launch renders the tiles tile_begin + k * tile_stride (k = 0 .. tile_count - 1) of the raster grid. A chunk is 64
    // consecutive iterations of one tile; every tile owns chunks_per_tile chunk numbers (the count a full tile_size^2 tile
    // needs: tiles cut by the image border leave their last ones empty), so chunk c belongs to the launch's tile
    // c / chunks_per_tile. [chunk_begin, chunk_end) is the range this launch renders (progress slices cut it). Wave w of the
    // persistent grid takes the chunks chunk_begin + w, + total_waves, ...: the stage scheduler's builds without interpreter programs
    // start a chunk's 64 samples at once, at full width, into the wave's start_queue and any lane of the wave may render them; in every
    // other build lane l of the wave renders iteration 64 * within + l of each of those chunks.
    uint32_t tile_begin, tile_stride, tile_count;
    uint32_t chunks_per_tile;
    uint32_t chunk_begin, chunk_end;
    uint32_t film_layout; // PYR_FILM_ROWS: film_out holds pixel rows [film_row_begin, + film_row_count); PYR_FILM_TILE_BLOCKS: one ringed block per tile
    uint32_t film_row_begin, film_row_count;
    uint64_t seed;
    float grains_per_wavelength; // bins / wl_width (film.rs:38)
    PyrGrain* film_out;
    unsigned long long* counters; // 9 words (PyrCounters order) or nullptr
    uint32_t scheduler; // 0 = bounce-synchronous walk (render_kernel), 1 = stage-scheduled state machine (render_kernel_sm)
    uint32_t sm_phase_lanes, sm_trav_steps; // stage scheduler: lanes that make a phase run; traversal steps per turn
    uint32_t sm_expose_lanes;               // finished lanes that make the tape replay run (TAPE builds)
    uint32_t stack_lds; // traversal stack levels kept in LDS (set by launch_render; deeper levels spill to scratch in the sm kernel)
    // Spectral tape of the stage-scheduled kernel (kernels.hip "Spectral tape"): [tape_max_ops][tape_lanes] 8-byte records,
    // one column per lane of the persistent grid.
    unsigned long long* tape;
    uint32_t tape_lanes, tape_max_ops;
    uint32_t* tape_overflow; // device word, set when a path wanted to append more than tape_max_ops records
    uint32_t tape_programs_lds; // programs whose prepared form the kernel keeps in LDS for the replay (set by launch_render; 0 = none)
    uint32_t sample_begin; // first sample of every pixel's budget this launch renders (PyrRenderParams::sample_begin); only locate_chunk reads it
    // Ready sample starts of the stage scheduler's builds without interpreter programs (kernels.hip Walker::expose_and_restart): one
    // slab of start_queue_stride words per wave of the persistent grid (tape_lanes / 64 of them), a ring laid out
    // [start_queue_words][kStartQueueEntries]. Empty at the start and at the end of every launch.
    uint32_t* start_queue;
    uint32_t start_queue_stride;
};

// PYR_SAMPLE_QUEUE=0 builds (A/B, tools/ab.sh) start every sample in the lane that renders it, as the interpreter builds do.
#ifndef PYR_SAMPLE_QUEUE
#define PYR_SAMPLE_QUEUE 1
#endif
// A ready start: the RNG state behind the start's draws (4 words), the film pixel, the camera ray (6), the S - 1 companion
// wavelengths and the hero wavelength. A wave fills at most 64 entries, and only while fewer than 64 are ready.
constexpr uint32_t kStartQueueEntries = 128, kStartQueueFixedWords = 11;
constexpr uint32_t start_queue_words(uint32_t spectrum_samples) { return kStartQueueFixedWords + spectrum_samples; }

// Work feed of the persistent traversal kernels: kFeedSegments cursor words, kFeedCursorStride words apart (kernels.hip WorkFeed).
constexpr uint32_t kFeedSegments = 8, kFeedCursorStride = 64;
constexpr size_t kFeedBytes = (size_t)kFeedSegments * kFeedCursorStride * sizeof(uint32_t);

struct IntersectLaunch {
    const float* rays;
    PyrHit* hits;
    uint32_t n;
    unsigned long long* counters;
    uint32_t* next;  // device, kFeedBytes, zero at launch: the work-feed cursors of the batch
    uint32_t num_cus;
    uint32_t reserve; // rays a wave reserves per atomic (set by launch_intersect)
    uint32_t stack_lds; // traversal stack levels kept in LDS (set by launch_intersect)
};

struct DevelopLaunch {
    PyrFilmDesc film;
    const PyrGrain* grains; // device
    float step_size, xyz_scale;
    uint32_t sample_count;
    const float* filter;    // device or nullptr
    const float* white_div; // device or nullptr
    const float* white_mul;
    const float* xyz_table; // device
    uint32_t xyz_count;
    float xyz_min, xyz_max;
    uint8_t* rgb_out; // device
    const PyrGrain* grains_b; // device or nullptr: a second half film, developed as grains + grains_b (develop_wave_kernel only)
};
// A launcher that refuses a launch, or whose launch fails, says why through fail() (api_internal.h) and returns that code.
int launch_develop(const DevelopLaunch& launch, void* stream); // develop_kernel: one thread per pixel (kernels/main.hip)

// kernels/film.hip: the kernels of a progressive session's film
// develop_wave_kernel: one wave per run of 64 pixels, the same bytes as develop_kernel. Its LDS rows hold films of up to
// kWaveDevelopMaxBins bins (64 KB a wave); develop_wave_serves says whether a launch fits, launch_develop_wave refuses one that does not.
constexpr uint32_t kWaveDevelopMaxBins = 255;
bool develop_wave_serves(const DevelopLaunch& launch);
int launch_develop_wave(const DevelopLaunch& launch, void* stream);
int launch_film_sum(const PyrGrain* a, const PyrGrain* b, PyrGrain* out, size_t grains, void* stream); // out = a + b (out may be a or b)
struct NoiseLaunch {
    PyrFilmDesc film;
    uint32_t tile_size, tiles_x, tiles_y;
    const PyrGrain* a; // device, whole image: the two half films
    const PyrGrain* b;
    float* out; // device, tiles_x * tiles_y
};
int launch_noise(const NoiseLaunch& launch, void* stream);

// kernels/tone.hip: the film as an image in linear light, its luminance statistics, its tone mapping
struct LinearLaunch {
    DevelopLaunch develop; // rgb_out is not read; grains_b is served by both forms
    float* out;            // device, height * width * 3 floats
    uint32_t space;        // PYR_LINEAR_XYZ or PYR_LINEAR_SRGB
};
// develop_linear_kernel (a wave per run of 64 pixels) up to kWaveDevelopMaxBins bins, develop_linear_pixel_kernel beyond
int launch_develop_linear(const LinearLaunch& launch, void* stream);
// Zeroes `out` (device) and fills it from `image` (device, pixels * 3 floats, linear sRGB), all on `stream`.
int launch_image_stats(const float* image, size_t pixels, PyrImageStats* out, void* stream);
struct ToneLaunch {
    const float* image; // device, pixels * 3 floats, linear sRGB
    uint8_t* rgb_out;   // device, pixels * 3 bytes
    size_t pixels;
    uint32_t op; // PYR_TONE_CLIP or PYR_TONE_REINHARD
    float exposure, white;
};
int launch_tonemap(const ToneLaunch& launch, void* stream);

// kernels/denoise.hip: the cross filter of two developed half images. One launch filters `averaged` with
// the weights read from `weights_from`; the caller launches it twice with the halves exchanged and combines the two results.
struct DenoiseLaunch {
    const float* weights_from; // device, height * width * 3 floats: the half H of the colour distance
    const float* averaged;     // device, the other half
    const float* variance;     // device, height * width * 3 floats (launch_denoise_variance)
    const float* albedo;             // device, height * width * 3 floats, or nullptr
    const PyrFeaturePixel* pixels;   // device, height * width records, or nullptr
    uint32_t width, height, radius, patch;
    float kk, epsilon;                         // k * k
    float albedo_div, normal_div, depth_div;   // 2.0f * (sigma * sigma); <= 0: that guide is off
    float* out;       // device, height * width * 3 floats
    uint32_t tiles_x; // set by the launcher
};
int launch_denoise_variance(const float* a, const float* b, uint32_t width, uint32_t height, float* variance, void* stream);
int launch_denoise_filter(const DenoiseLaunch& launch, void* stream);
// out = (fa + fb) * 0.5f and, unless it is nullptr, error_out = fabsf(fa - fb) * 0.5f
int launch_denoise_combine(const float* fa, const float* fb, size_t pixels, float* out, float* error_out, void* stream);

// Adds the PYR_FILM_TILE_BLOCKS buffer of the tiles tile_begin + k * tile_stride (k < tile_count) into a whole-image film.
struct AssembleLaunch {
    PyrFilmDesc film;
    uint32_t tile_size, tiles_x;
    uint32_t tile_begin, tile_stride, tile_count;
    const PyrGrain* blocks; // device
    PyrGrain* film_out;     // device, whole image
};
int launch_assemble(const AssembleLaunch& launch, void* stream);

// kernels/features.hip: the first-hit feature pass. An item is a pixel; 64 consecutive items are an 8 x 8
// pixel square (the launcher numbers them and sets `n`, `squares_x`, `reserve` and `stack_lds`).
struct FeatureLaunch {
    PyrCamera camera; // aperture is not read: the lens is its centre
    PyrFilmDesc film; // width, height and the wavelength span; bins is not read
    uint32_t grid, albedo_bins;
    PyrGrain* albedo;        // device, height * width * albedo_bins grains, added into; or nullptr
    PyrFeaturePixel* pixels; // device, height * width records, overwritten; or nullptr
    uint32_t* next;          // device, kFeedBytes, zero at launch: the work-feed cursors
    uint32_t n, squares_x, reserve, stack_lds;
};
using FeatureKernel = void (*)(DevScene, FeatureLaunch);
FeatureKernel pick_wide_features_kernel(); // kernels/features_wide.hip: the build whose interpreter holds the wide register file
int launch_features(const DevScene& scene, const FeatureLaunch& launch, void* stream, int num_cus, bool wide_vm);

// kernels/motion.hip: the motion pass. Items are the feature pass's: a pixel each, 64 consecutive ones an
// 8 x 8 square (the launcher numbers them and sets `n`, `squares_x`, `reserve` and `stack_lds`). The snapshot of the previous
// frame's geometry travels here, not in DevScene: the render kernels take that struct by value and know nothing of this pass.
struct MotionLaunch {
    PyrCamera camera;            // aperture is not read: the lens is its centre
    float previous_w[16];        // pyr_camera_world_to_cam of the previous camera
    float previous_view_plane;
    uint32_t width, height;
    const float* previous_positions; // device, [triangles][3][3] in the description's order, or nullptr: no snapshot
    const float* previous_spheres;   // device, [spheres][4], or nullptr
    PyrMotionPixel* pixels;          // device, height * width records, overwritten
    uint32_t* next;                  // device, kFeedBytes, zero at launch: the work-feed cursors
    uint32_t n, squares_x, reserve, stack_lds;
};
int launch_motion(const DevScene& scene, const MotionLaunch& launch, void* stream, int num_cus);

// kernels/reproject.hip: accumulation over frames (pyrite_gpu.h "motion records and accumulation over frames")
struct ReprojectLaunch {
    const float* current;                 // device, height * width * 3 floats
    const PyrMotionPixel* motion;         // device, height * width records
    const float* history;                 // device, or all three nullptr: a first frame
    const PyrMotionPixel* history_motion;
    const float* history_count;
    uint32_t width, height;
    float depth_tolerance, max_history;
    float* out;       // device, height * width * 3 floats
    float* count_out; // device, height * width floats
};
int launch_reproject(const ReprojectLaunch& launch, void* stream);

// kernels/temporal.hip: the temporal resolve (pyrite_gpu.h "temporal resolve"): the reprojection's fetch, the
// history clipped to the neighbourhood of `current`
struct TemporalLaunch {
    const float* current;                 // device, height * width * 3 floats
    const PyrMotionPixel* motion;         // device, height * width records
    const float* noise;                   // device, height * width * 3 floats, or nullptr: the build that stages none
    const float* history;                 // device, or all three nullptr: a first frame
    const PyrMotionPixel* history_motion;
    const float* history_count;
    uint32_t width, height;
    float depth_tolerance, max_history;
    uint32_t radius; // 1..PYR_TEMPORAL_MOST_RADIUS
    float gamma, noise_scale, response;
    float* out;       // device, height * width * 3 floats
    float* count_out; // device, height * width floats
    float* clip_out;  // device, height * width floats, or nullptr
};
int launch_temporal(const TemporalLaunch& launch, void* stream);

// kernels/motion_blur.hip: motion blur over the motion records (pyrite_gpu.h "motion blur over the motion records", DESIGN.md
// section 9j). `work` is motion_blur_work_bytes() of device memory, 16-byte aligned, overwritten: four floats a pixel (hx, hy, len, z)
// and twice four a tile (the tile maxima, the neighbour maxima). Three launches on `stream`: velocity, neighbour maximum, gather.
struct MotionBlurLaunch {
    const float* image;           // device, height * width * 3 floats
    const PyrMotionPixel* motion; // device, height * width records
    uint32_t width, height;
    float shutter, depth_softness;
    uint32_t samples, max_radius, seed;
    float* work;
    float* out; // device, height * width * 3 floats; overlaps no input
};
size_t motion_blur_work_bytes(uint32_t width, uint32_t height, uint32_t max_radius);
int launch_motion_blur(const MotionBlurLaunch& launch, void* stream);

// kernels/glare.hip: the glare of a linear image (pyrite_gpu.h "glare"). `work` is glare_work_bytes() of
// device memory, 16-byte aligned, overwritten: levels 1..L of the pyramid, one after the other, four floats a pixel. L downs, L - 1
// ups and the compose on `stream`, the steps of the small levels in one launch (the tail); a 1 x 1 image is copied.
struct GlareLaunch {
    const float* image; // device, height * width * 3 floats
    uint32_t width, height;
    float strength, threshold, falloff;
    uint32_t levels; // as given: 1..PYR_GLARE_MOST_LEVELS; the launcher takes the smaller of it and what the image has
    float* work;
    float* out; // device, height * width * 3 floats; does not overlap image
};
size_t glare_work_bytes(uint32_t width, uint32_t height, uint32_t levels);
int launch_glare(const GlareLaunch& launch, void* stream);

// kernels/upsample.hip: the guided upsampling of a low-resolution linear image (pyrite_gpu.h "upsample").
// One launch on `stream`, no working memory. Either pair is null or given whole.
struct UpsampleLaunch {
    const float* low;                  // device, low_height * low_width * 3 floats
    const float* low_albedo;           // device, the same size, or null
    const PyrFeaturePixel* low_pixels; // device, 16-byte aligned, or null
    uint32_t low_width, low_height, scale;
    const float* albedo;           // device, scale*low_height * scale*low_width * 3 floats, or null
    const PyrFeaturePixel* pixels; // device, 16-byte aligned, or null
    uint32_t radius;               // 1..PYR_UPSAMPLE_MOST_RADIUS
    uint32_t use_normal, use_depth, match_material; // the guide switches: wave-uniform
    float normal_div, depth_div;   // 2.0f * (sigma * sigma), formed on the host in f32
    float albedo_floor, max_gain;
    float* out; // device, scale*low_height * scale*low_width * 3 floats
};
int launch_upsample(const UpsampleLaunch& launch, void* stream);

// kernels/despeckle.hip: the firefly clamp of one or two half images (pyrite_gpu.h "despeckle"). The counts
// are zeroed and one kernel is launched on `stream`; no working memory. No output overlaps an input or another output.
struct DespeckleLaunch {
    const float* a; // device, height * width * 3 floats
    const float* b; // device, the same size, or null: one image, no agreement test
    uint32_t width, height;
    uint32_t radius; // 1..PYR_DESPECKLE_MOST_RADIUS
    float k, relative, floor;
    float* a_out;     // device, the size of a
    float* b_out;     // device, given with b
    float* removed;   // device, the size of a, or null
    uint32_t* counts; // device, two words, or null
    uint32_t tiles_x; // the launcher's
};
int launch_despeckle(const DespeckleLaunch& launch, void* stream);

// kernels/lens_blur.hip: lens blur over the feature records (pyrite_gpu.h "lens blur over the feature records", DESIGN.md section
// 9o). One launch on `stream`, no working memory.
struct LensBlurLaunch {
    const float* image;            // device, height * width * 3 floats
    const PyrFeaturePixel* pixels; // device, height * width records, 16-byte aligned
    uint32_t width, height;
    float focus_distance, aperture, view_plane, depth_tolerance;
    uint32_t max_radius; // 1..PYR_LENS_BLUR_MOST_RADIUS
    float* out;          // device, height * width * 3 floats; overlaps no input
};
int launch_lens_blur(const LensBlurLaunch& launch, void* stream);

// launchers (kernels/main.hip)
// wide_vm: the scene has a program that only the wide interpreter build (kernels/wide.hip) holds
int launch_render(const DevScene& scene, const RenderLaunch& launch, bool with_counters, void* stream, int num_cus, bool wide_vm = false);
uint32_t tape_ops_bound(const DevScene& scene, const RenderLaunch& launch); // records per path the stage-scheduled kernel may append to its spectral tape
uint32_t launch_tape(const DevScene& scene, const RenderLaunch& launch); // the tape this launch records, as PyrPathInfo::tape counts: 0 none, 1 spectral, 2 hit tape
uint32_t tape_lanes_bound(int num_cus);              // lanes (tape columns) of the largest grid launch_render starts
int launch_intersect(const DevScene& scene, const IntersectLaunch& launch, bool with_counters, void* stream);
bool scene_is_lds_resident(const DevScene& scene);
// Which unit under kernels/ holds which build of render_kernel_sm: main.hip's pick_kernel asks these, each defined by the unit it is
// named after (pick_wide_kernel: nullptr in the one-unit build, kernels/profile.hip).
using RenderKernel = void (*)(DevScene, RenderLaunch);
RenderKernel pick_interp_kernel(bool with_counters, bool lds_scene, bool lds_tables, bool hit_tape, bool product);
RenderKernel pick_product_kernel(bool with_counters, bool lds_scene, bool lds_tables);
RenderKernel pick_wide_kernel(bool with_counters, bool lds_scene, bool lds_tables);

} // namespace pyr
