"""ctypes mirror of include/pyrite_gpu.h (the C ABI). Field order and widths must match the header exactly;
tests/test_abi.py checks sizes and that every declared symbol is exported."""
import ctypes as C

PYR_ABI_VERSION = 5

PYR_OK = 0
PYR_ERR_INVALID_ARGUMENT = -1
PYR_ERR_UNSUPPORTED = -2
PYR_ERR_DEVICE = -3
PYR_ERR_OUT_OF_MEMORY = -4

PYR_FLAG_COUNTERS = 1
PYR_FILM_ROWS, PYR_FILM_TILE_BLOCKS = 0, 1
PYR_SESSION_HALVES = 1
PYR_COMM_ID_BYTES = 128

# PyrOp
OP_NUMBER, OP_VECTOR, OP_RGB, OP_SPECTRUM, OP_COLOR_TEXTURE, OP_MONO_TEXTURE, OP_RGB_SPECTRUM = range(7)
OP_FRESNEL, OP_BLACKBODY, OP_RGB_TO_VECTOR, OP_BINARY, OP_MIX, OP_CLAMP = range(7, 13)
VT_NUMBER, VT_VECTOR, VT_RGB = 0, 1, 2
BIN_ADD, BIN_SUB, BIN_MUL, BIN_DIV = 0, 1, 2, 3
OPERAND_CONSTANT, OPERAND_INPUT, OPERAND_REGISTER = 0, 1, 2
INPUT_WAVELENGTH = 0
INPUT_NORMAL, INPUT_INCIDENT, INPUT_TEXTURE = 0, 1, 2
DEP_WAVELENGTH, DEP_NORMAL, DEP_INCIDENT, DEP_TEXTURE = 0x01, 0x10, 0x20, 0x40
PROGRAM_CONSTANT, PROGRAM_INSTRUCTIONS = 0, 1
OUTPUT_NUMBER, OUTPUT_VECTOR = 0, 1
SPECTRUM_ARRAY, SPECTRUM_CURVE = 0, 1
BSDF_EMISSIVE, BSDF_DIFFUSE, BSDF_MIRROR, BSDF_REFRACTIVE = 0, 1, 2, 3
LAMP_DIRECTIONAL, LAMP_POINT, LAMP_SHAPE = 0, 1, 2
SHAPE_SPHERE, SHAPE_TRIANGLE, SHAPE_PLANE = 0, 1, 2
HIT_NONE = 0xFFFFFFFF

MAX_NUMBER_REGISTERS, MAX_VECTOR_REGISTERS, MAX_RGB_REGISTERS = 16, 8, 8
WIDE_NUMBER_REGISTERS, WIDE_VECTOR_REGISTERS, WIDE_RGB_REGISTERS = 64, 32, 32
MAX_DECLARED_REGISTERS = 65536


class PyrGrain(C.Structure):
    _fields_ = [("acc", C.c_float), ("weight", C.c_float)]


class PyrFilmDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bins", C.c_uint32), ("wl_start", C.c_float), ("wl_width", C.c_float)]


class PyrRenderParams(C.Structure):
    _fields_ = [
        ("bounces", C.c_uint32),
        ("pixel_samples", C.c_uint32),
        ("light_samples", C.c_uint32),
        ("spectrum_samples", C.c_uint32),
        ("tile_size", C.c_uint32),
        ("flags", C.c_uint32),
        ("seed", C.c_uint64),
        ("tile_begin", C.c_uint32),
        ("tile_end", C.c_uint32),
        ("film_row_begin", C.c_uint32),
        ("film_row_count", C.c_uint32),
        ("tile_stride", C.c_uint32),
        ("film_layout", C.c_uint32),
        ("sample_begin", C.c_uint32),
    ]


class PyrCamera(C.Structure):
    _fields_ = [("cam_to_world", C.c_float * 16), ("view_plane", C.c_float), ("focus_distance", C.c_float), ("aperture", C.c_float)]


class PyrOperand(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("bits", C.c_uint32)]


class PyrInstr(C.Structure):
    _fields_ = [
        ("op", C.c_uint32),
        ("value_type", C.c_uint32),
        ("operator_", C.c_uint32),
        ("deps", C.c_uint32),
        ("output", C.c_uint32),
        ("a", C.c_uint32),
        ("b", C.c_uint32),
        ("reserved", C.c_uint32),
        ("x", PyrOperand),
        ("y", PyrOperand),
        ("z", PyrOperand),
        ("w", PyrOperand),
    ]


class PyrProgram(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("constant", C.c_float),
        ("first_instr", C.c_uint32),
        ("num_instrs", C.c_uint32),
        ("output_kind", C.c_uint32),
        ("output_reg", C.c_uint32),
        ("num_numbers", C.c_uint32),
        ("num_vectors", C.c_uint32),
        ("num_rgbs", C.c_uint32),
    ]


class PyrSpectrum(C.Structure):
    _fields_ = [("format", C.c_uint32), ("min", C.c_float), ("max", C.c_float), ("offset", C.c_uint32), ("count", C.c_uint32)]


class PyrComponent(C.Structure):
    _fields_ = [
        ("bsdf", C.c_uint32),
        ("color_program", C.c_uint32),
        ("probability_program", C.c_int32),
        ("selection_compensation", C.c_float),
        ("ior", C.c_float),
        ("env_ior", C.c_float),
        ("dispersion", C.c_float),
        ("env_dispersion", C.c_float),
    ]


class PyrMaterial(C.Structure):
    _fields_ = [
        ("first_component", C.c_uint32),
        ("num_components", C.c_uint32),
        ("first_emissive", C.c_uint32),
        ("num_emissive", C.c_uint32),
        ("normal_map_program", C.c_int32),
    ]


class PyrLamp(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("shape_kind", C.c_uint32),
        ("shape_index", C.c_uint32),
        ("color_program", C.c_uint32),
        ("v", C.c_float * 3),
        ("width", C.c_float),
    ]


class PyrTexture(C.Structure):
    _fields_ = [("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("reserved", C.c_uint32), ("offset", C.c_uint64)]


TEXTURE_COLOR, TEXTURE_MONO = 0, 1

_fp = C.POINTER(C.c_float)
_up = C.POINTER(C.c_uint32)


class PyrSceneDesc(C.Structure):
    _fields_ = [
        ("num_triangles", C.c_uint32),
        ("tri_positions", _fp),
        ("tri_normals", _fp),
        ("tri_uvs", _fp),
        ("tri_material", _up),
        ("num_spheres", C.c_uint32),
        ("spheres", _fp),
        ("sphere_tex_scale", _fp),
        ("sphere_material", _up),
        ("num_planes", C.c_uint32),
        ("planes", _fp),
        ("plane_material", _up),
        ("num_lamps", C.c_uint32),
        ("lamps", C.POINTER(PyrLamp)),
        ("num_materials", C.c_uint32),
        ("materials", C.POINTER(PyrMaterial)),
        ("num_components", C.c_uint32),
        ("components", C.POINTER(PyrComponent)),
        ("num_programs", C.c_uint32),
        ("programs", C.POINTER(PyrProgram)),
        ("num_instrs", C.c_uint32),
        ("instrs", C.POINTER(PyrInstr)),
        ("num_spectra", C.c_uint32),
        ("spectra", C.POINTER(PyrSpectrum)),
        ("num_spectrum_floats", C.c_uint32),
        ("spectrum_data", _fp),
        ("rgb_basis", _fp),
        ("rgb_basis_count", C.c_uint32),
        ("rgb_basis_min", C.c_float),
        ("rgb_basis_max", C.c_float),
        ("sky_program", C.c_uint32),
        ("num_textures", C.c_uint32),
        ("textures", C.POINTER(PyrTexture)),
        ("num_texture_floats", C.c_uint64),
        ("texture_data", _fp),
        ("tri_frames", _fp),
        ("plane_frames", _fp),
    ]


class PyrCounters(C.Structure):
    _fields_ = [
        ("samples", C.c_uint64),
        ("extension_rays", C.c_uint64),
        ("shadow_rays", C.c_uint64),
        ("box_tests", C.c_uint64),
        ("triangle_tests", C.c_uint64),
        ("sphere_tests", C.c_uint64),
        ("plane_tests", C.c_uint64),
        ("shaded_hits", C.c_uint64),
        ("exposures", C.c_uint64),
    ]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class PyrHit(C.Structure):
    _fields_ = [("distance", C.c_float), ("shape", C.c_uint32), ("u", C.c_float), ("v", C.c_float)]


class PyrBvhInfo(C.Structure):
    _fields_ = [
        ("num_nodes", C.c_uint32),
        ("num_leaves", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("num_primitives", C.c_uint32),
        ("node_bytes", C.c_uint64),
        ("primitive_bytes", C.c_uint64),
        ("num_wide_nodes", C.c_uint32),
        ("num_pair_records", C.c_uint32),
        ("wide_node_bytes", C.c_uint64),
        ("pair_record_bytes", C.c_uint64),
    ]


PYR_BUILD_HOST = 0
PYR_BUILD_DEVICE = 1
PYR_BUILD_FALLBACK_NONE = 0
PYR_BUILD_FALLBACK_SPATIAL_SPLITS = 1
PYR_BUILD_FALLBACK_MEDIAN_TOO_LARGE = 2
PYR_BUILD_FALLBACK_INTERNAL = 3


class PyrBuildParams(C.Structure):
    _fields_ = [
        ("builder", C.c_uint32),
        ("reserved", C.c_uint32 * 7),
    ]


class PyrBuildInfo(C.Structure):
    _fields_ = [
        ("builder_asked", C.c_uint32),
        ("builder_used", C.c_uint32),
        ("fallback_reason", C.c_uint32),
        ("levels", C.c_uint32),
        ("median_splits", C.c_uint32),
        ("reserved", C.c_uint32),
        ("tree_digest", C.c_uint64),
        ("bounds_ms", C.c_float),
        ("tree_ms", C.c_float),
        ("finish_ms", C.c_float),
        ("collapse_ms", C.c_float),
        ("pack_upload_ms", C.c_float),
        ("total_ms", C.c_float),
    ]


PYR_UPDATE_REFIT = 0
PYR_UPDATE_REBUILD = 1
PYR_SKIN_LINEAR = 0
PYR_SKIN_DUAL_QUATERNION = 1


class PyrGeometryUpdate(C.Structure):
    _fields_ = [
        ("mode", C.c_uint32),
        ("num_triangles", C.c_uint32),
        ("num_spheres", C.c_uint32),
        ("tri_positions", C.c_void_p),
        ("tri_normals", C.c_void_p),
        ("tri_frames", C.c_void_p),
        ("spheres", C.c_void_p),
        ("reserved", C.c_uint32 * 4),
    ]


class PyrUpdateInfo(C.Structure):
    _fields_ = [
        ("mode_used", C.c_uint32),
        ("levels", C.c_uint32),
        ("updates", C.c_uint32),
        ("upload_ms", C.c_float),
        ("prims_ms", C.c_float),
        ("refit_ms", C.c_float),
        ("total_ms", C.c_float),
        ("area_ratio", C.c_double),
        ("reserved", C.c_uint32 * 4),
    ]


class PyrObjectRange(C.Structure):
    _fields_ = [
        ("first_triangle", C.c_uint32),
        ("num_triangles", C.c_uint32),
        ("first_sphere", C.c_uint32),
        ("num_spheres", C.c_uint32),
    ]


class PyrObjectPose(C.Structure):
    _fields_ = [
        ("transform", C.c_float * 16),
        ("scale", C.c_float),
        ("reserved", C.c_uint32 * 3),
    ]


class PyrPoseUpdate(C.Structure):
    _fields_ = [
        ("mode", C.c_uint32),
        ("num_objects", C.c_uint32),
        ("poses", C.POINTER(PyrObjectPose)),
        ("reserved", C.c_uint32 * 4),
    ]


class PyrSkin(C.Structure):
    _fields_ = [
        ("object", C.c_uint32),
        ("num_joints", C.c_uint32),
        ("joints", C.c_void_p),
        ("weights", C.c_void_p),
        ("reserved", C.c_uint32 * 4),
    ]


class PyrSkinUpdate(C.Structure):
    _fields_ = [
        ("mode", C.c_uint32),
        ("num_objects", C.c_uint32),
        ("poses", C.POINTER(PyrObjectPose)),
        ("joints", C.c_void_p),
        ("num_joints", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class PyrMorph(C.Structure):
    _fields_ = [
        ("object", C.c_uint32),
        ("num_targets", C.c_uint32),
        ("position_deltas", C.c_void_p),
        ("normal_deltas", C.c_void_p),
        ("reserved", C.c_uint32 * 4),
    ]


class PyrMorphUpdate(C.Structure):
    _fields_ = [
        ("mode", C.c_uint32),
        ("num_objects", C.c_uint32),
        ("poses", C.POINTER(PyrObjectPose)),
        ("joints", C.c_void_p),
        ("num_joints", C.c_uint32),
        ("weights", C.c_void_p),
        ("num_weights", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class PyrSmoothing(C.Structure):
    _fields_ = [
        ("object", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("vertex_ids", C.c_void_p),
        ("reserved", C.c_uint32 * 4),
    ]


class PyrPathInfo(C.Structure):
    _fields_ = [
        ("stage_scheduler", C.c_uint32),
        ("interpreter", C.c_uint32),
        ("scene_in_lds", C.c_uint32),
        ("tape", C.c_uint32),
        ("phase_lanes", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class PyrProgramInfo(C.Structure):
    _fields_ = [
        ("declared_numbers", C.c_uint32),
        ("declared_vectors", C.c_uint32),
        ("declared_rgbs", C.c_uint32),
        ("allocated_numbers", C.c_uint32),
        ("allocated_vectors", C.c_uint32),
        ("allocated_rgbs", C.c_uint32),
        ("wide", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class PyrDevelopParams(C.Structure):
    _fields_ = [
        ("step_size", C.c_float),
        ("xyz_scale", C.c_float),
        ("sample_count", C.c_uint32),
        ("filter", _fp),
        ("white_div", _fp),
        ("white_mul", _fp),
        ("xyz_table", _fp),
        ("xyz_count", C.c_uint32),
        ("xyz_min", C.c_float),
        ("xyz_max", C.c_float),
    ]


class PyrFeatureParams(C.Structure):
    _fields_ = [("grid", C.c_uint32), ("albedo_bins", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PyrFeaturePixel(C.Structure):
    _fields_ = [
        ("normal", C.c_float * 3),
        ("depth", C.c_float),
        ("coverage", C.c_float),
        ("shape", C.c_uint32),
        ("material", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


PYR_LINEAR_XYZ, PYR_LINEAR_SRGB = 0, 1
PYR_TONE_CLIP, PYR_TONE_REINHARD = 0, 1
PYR_TONE_KEY, PYR_TONE_PERCENTILE, PYR_TONE_WHITE_PERCENTILE = 0.18, 0.5, 0.99


class PyrImageStats(C.Structure):
    _fields_ = [("histogram", C.c_uint32 * 256), ("lit", C.c_uint32), ("dark", C.c_uint32), ("min_lit", C.c_float), ("max_lit", C.c_float)]

    def as_dict(self):
        return {"histogram": list(self.histogram), "lit": int(self.lit), "dark": int(self.dark), "min_lit": float(self.min_lit), "max_lit": float(self.max_lit)}


class PyrToneParams(C.Structure):
    _fields_ = [
        ("op", C.c_uint32),
        ("exposure", C.c_float),
        ("white", C.c_float),
        ("key", C.c_float),
        ("percentile", C.c_float),
        ("white_percentile", C.c_float),
    ]


PYR_DENOISE_RADIUS, PYR_DENOISE_PATCH, PYR_DENOISE_K, PYR_DENOISE_EPSILON = 5, 1, 0.45, 1e-10
PYR_DENOISE_SIGMA_ALBEDO, PYR_DENOISE_SIGMA_NORMAL, PYR_DENOISE_SIGMA_DEPTH = 0.02, 0.1, 0.02
PYR_DENOISE_MAX_RADIUS, PYR_DENOISE_MAX_PATCH = 10, 3


class PyrDenoiseParams(C.Structure):
    _fields_ = [
        ("radius", C.c_uint32),
        ("patch", C.c_uint32),
        ("k", C.c_float),
        ("epsilon", C.c_float),
        ("sigma_albedo", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_depth", C.c_float),
        ("reserved", C.c_uint32),
    ]


PYR_MOTION_HIT, PYR_MOTION_IN_FRONT, PYR_MOTION_INSIDE = 1, 2, 4
PYR_REPROJECT_DEPTH_TOLERANCE, PYR_REPROJECT_MAX_HISTORY = 0.02, 32.0


class PyrMotionPixel(C.Structure):
    _fields_ = [
        ("prev_x", C.c_float),
        ("prev_y", C.c_float),
        ("prev_depth", C.c_float),
        ("depth", C.c_float),
        ("shape", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class PyrReprojectParams(C.Structure):
    _fields_ = [("depth_tolerance", C.c_float), ("max_history", C.c_float), ("reserved", C.c_uint32 * 2)]


PYR_MOTION_BLUR_SHUTTER, PYR_MOTION_BLUR_SAMPLES, PYR_MOTION_BLUR_MAX_RADIUS, PYR_MOTION_BLUR_DEPTH_SOFTNESS = 0.5, 15, 16, 0.02
PYR_MOTION_BLUR_MOST_SAMPLES, PYR_MOTION_BLUR_MOST_RADIUS = 64, 64


class PyrMotionBlurParams(C.Structure):
    _fields_ = [("shutter", C.c_float), ("samples", C.c_uint32), ("max_radius", C.c_uint32), ("depth_softness", C.c_float), ("seed", C.c_uint32), ("reserved", C.c_uint32 * 3)]


PYR_TEMPORAL_RADIUS, PYR_TEMPORAL_GAMMA, PYR_TEMPORAL_NOISE_SCALE, PYR_TEMPORAL_RESPONSE, PYR_TEMPORAL_MOST_RADIUS = 1, 1.0, 1.0, 1.0, 3


class PyrTemporalParams(C.Structure):
    _fields_ = [("depth_tolerance", C.c_float), ("max_history", C.c_float), ("radius", C.c_uint32), ("gamma", C.c_float), ("noise_scale", C.c_float),
                ("response", C.c_float), ("reserved", C.c_uint32 * 2)]


PYR_GLARE_STRENGTH, PYR_GLARE_LEVELS, PYR_GLARE_THRESHOLD, PYR_GLARE_FALLOFF, PYR_GLARE_MOST_LEVELS = 0.1, 6, 0.0, 1.0, 12


class PyrGlareParams(C.Structure):
    _fields_ = [("strength", C.c_float), ("levels", C.c_uint32), ("threshold", C.c_float), ("falloff", C.c_float), ("reserved", C.c_uint32 * 4)]


PYR_UPSAMPLE_RADIUS, PYR_UPSAMPLE_MOST_RADIUS, PYR_UPSAMPLE_MOST_SCALE, PYR_UPSAMPLE_MATCH_MATERIAL = 1, 3, 8, 1
PYR_UPSAMPLE_SIGMA_NORMAL, PYR_UPSAMPLE_SIGMA_DEPTH, PYR_UPSAMPLE_ALBEDO_FLOOR, PYR_UPSAMPLE_MAX_GAIN = 0.1, 0.02, 0.01, 4.0


class PyrUpsampleParams(C.Structure):
    _fields_ = [("radius", C.c_uint32), ("flags", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("albedo_floor", C.c_float),
                ("max_gain", C.c_float), ("reserved", C.c_uint32 * 2)]


PYR_DESPECKLE_RADIUS, PYR_DESPECKLE_MOST_RADIUS, PYR_DESPECKLE_K, PYR_DESPECKLE_RELATIVE, PYR_DESPECKLE_FLOOR, PYR_DESPECKLE_LEAST_SAMPLES = 2, 2, 6.0, 0.1, 1e-4, 5


class PyrDespeckleParams(C.Structure):
    _fields_ = [("radius", C.c_uint32), ("k", C.c_float), ("relative", C.c_float), ("floor", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


PYR_LENS_BLUR_MAX_RADIUS, PYR_LENS_BLUR_MOST_RADIUS = 8, 16


class PyrLensBlurParams(C.Structure):
    _fields_ = [("focus_distance", C.c_float), ("aperture", C.c_float), ("view_plane", C.c_float), ("max_radius", C.c_uint32), ("depth_tolerance", C.c_float),
                ("reserved", C.c_uint32 * 3)]


PyrProgressFn = C.CFUNCTYPE(None, C.c_void_p, C.c_uint8, C.c_char_p)
PyrPreviewFn = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_uint32)

# Every entry point include/pyrite_gpu.h declares: name -> (restype, argtypes)
ENTRY_POINTS = {
    "pyr_abi_version": (C.c_int, []),
    "pyr_device_count": (C.c_int, []),
    "pyr_last_error": (C.c_char_p, []),
    "pyr_scene_create": (C.c_int, [C.POINTER(PyrSceneDesc), C.c_int, C.POINTER(C.c_void_p)]),
    "pyr_scene_destroy": (None, [C.c_void_p]),
    "pyr_render_simple": (
        C.c_int,
        [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.POINTER(PyrRenderParams), C.c_void_p, PyrProgressFn, C.c_void_p],
    ),
    "pyr_render_simple_device": (
        C.c_int,
        [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.POINTER(PyrRenderParams), C.c_void_p, C.c_void_p],
    ),
    "pyr_scene_counters": (C.c_int, [C.c_void_p, C.POINTER(PyrCounters)]),
    "pyr_scene_intersect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(PyrCounters)]),
    "pyr_scene_intersect_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pyr_scene_bvh_info": (C.c_int, [C.c_void_p, C.POINTER(PyrBvhInfo)]),
    "pyr_scene_create_with": (C.c_int, [C.POINTER(PyrSceneDesc), C.c_int, C.POINTER(PyrBuildParams), C.POINTER(C.c_void_p)]),
    "pyr_scene_build_info": (C.c_int, [C.c_void_p, C.POINTER(PyrBuildInfo)]),
    "pyr_scene_update": (C.c_int, [C.c_void_p, C.POINTER(PyrGeometryUpdate)]),
    "pyr_scene_update_device": (C.c_int, [C.c_void_p, C.POINTER(PyrGeometryUpdate), C.c_void_p]),
    "pyr_scene_update_info": (C.c_int, [C.c_void_p, C.POINTER(PyrUpdateInfo)]),
    "pyr_scene_set_objects": (C.c_int, [C.c_void_p, C.POINTER(PyrObjectRange), C.c_uint32]),
    "pyr_scene_pose": (C.c_int, [C.c_void_p, C.POINTER(PyrPoseUpdate), C.c_void_p]),
    "pyr_scene_geometry": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pyr_scene_set_skins": (C.c_int, [C.c_void_p, C.POINTER(PyrSkin), C.c_uint32]),
    "pyr_scene_set_skin_blend": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]),
    "pyr_scene_skin": (C.c_int, [C.c_void_p, C.POINTER(PyrSkinUpdate), C.c_void_p]),
    "pyr_scene_set_morphs": (C.c_int, [C.c_void_p, C.POINTER(PyrMorph), C.c_uint32]),
    "pyr_scene_morph": (C.c_int, [C.c_void_p, C.POINTER(PyrMorphUpdate), C.c_void_p]),
    "pyr_scene_set_smoothing": (C.c_int, [C.c_void_p, C.POINTER(PyrSmoothing), C.c_uint32]),
    "pyr_scene_path_info": (C.c_int, [C.c_void_p, C.POINTER(PyrRenderParams), C.POINTER(PyrPathInfo)]),
    "pyr_scene_program_info": (C.c_int, [C.c_void_p, C.POINTER(PyrProgramInfo)]),
    "pyr_program_allocate_registers": (C.c_int, [C.POINTER(PyrInstr), C.POINTER(PyrProgram), C.POINTER(PyrInstr), C.POINTER(PyrProgram)]),
    "pyr_film_blocks_grains": (C.c_uint64, [C.POINTER(PyrFilmDesc), C.POINTER(PyrRenderParams)]),
    "pyr_film_blocks_assemble_device": (C.c_int, [C.POINTER(PyrFilmDesc), C.POINTER(PyrRenderParams), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pyr_comm_unique_id": (C.c_int, [C.c_void_p]),
    "pyr_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "pyr_comm_destroy": (None, [C.c_void_p]),
    "pyr_comm_uses_rccl": (C.c_int, [C.c_void_p]),
    "pyr_comm_status": (C.c_int, [C.c_void_p]),
    "pyr_render_simple_sharded": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.POINTER(PyrRenderParams), C.c_void_p, C.c_void_p],
    ),
    "pyr_render_simple_multi": (
        C.c_int,
        [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.POINTER(PyrRenderParams), C.c_void_p, PyrProgressFn, C.c_void_p],
    ),
    "pyr_film_develop": (C.c_int, [C.POINTER(PyrFilmDesc), C.c_void_p, C.POINTER(PyrDevelopParams), C.c_void_p, C.c_int]),
    "pyr_film_develop_device": (C.c_int, [C.POINTER(PyrFilmDesc), C.c_void_p, C.POINTER(PyrDevelopParams), C.c_void_p, C.c_int, C.c_void_p]),
    "pyr_session_create": (
        C.c_int,
        [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.POINTER(PyrRenderParams), C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)],
    ),
    "pyr_session_destroy": (None, [C.c_void_p]),
    "pyr_session_render": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pyr_session_sync": (C.c_int, [C.c_void_p]),
    "pyr_session_samples_done": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "pyr_session_preview": (C.c_int, [C.c_void_p, C.POINTER(PyrDevelopParams), C.c_void_p]),
    "pyr_session_film": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pyr_session_film_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pyr_session_halves": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pyr_session_noise": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pyr_render_simple_progressive": (
        C.c_int,
        [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.POINTER(PyrRenderParams), C.c_void_p, C.c_uint32, PyrProgressFn, PyrPreviewFn,
         C.c_double, C.POINTER(PyrDevelopParams), C.c_void_p],
    ),
    "pyr_render_features": (C.c_int, [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.POINTER(PyrFeatureParams), C.c_void_p, C.c_void_p]),
    "pyr_render_features_device": (
        C.c_int,
        [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.POINTER(PyrFeatureParams), C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "pyr_session_features": (C.c_int, [C.c_void_p, C.POINTER(PyrFeatureParams), C.c_void_p, C.c_void_p]),
    "pyr_film_develop_linear": (C.c_int, [C.POINTER(PyrFilmDesc), C.c_void_p, C.c_void_p, C.POINTER(PyrDevelopParams), C.c_uint32, C.c_void_p, C.c_int]),
    "pyr_film_develop_linear_device": (
        C.c_int,
        [C.POINTER(PyrFilmDesc), C.c_void_p, C.c_void_p, C.POINTER(PyrDevelopParams), C.c_uint32, C.c_void_p, C.c_int, C.c_void_p],
    ),
    "pyr_image_stats": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrImageStats), C.c_int]),
    "pyr_image_stats_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]),
    "pyr_tone_resolve": (C.c_int, [C.POINTER(PyrImageStats), C.POINTER(PyrToneParams), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pyr_image_tonemap": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrToneParams), C.c_void_p, C.c_int]),
    "pyr_image_tonemap_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrToneParams), C.c_void_p, C.c_int, C.c_void_p]),
    "pyr_session_linear": (C.c_int, [C.c_void_p, C.POINTER(PyrDevelopParams), C.c_uint32, C.c_void_p]),
    "pyr_session_preview_tone": (C.c_int, [C.c_void_p, C.POINTER(PyrDevelopParams), C.POINTER(PyrToneParams), C.c_void_p, C.POINTER(PyrImageStats)]),
    "pyr_image_denoise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrDenoiseParams), C.c_void_p, C.c_void_p, C.c_int]),
    "pyr_image_denoise_device": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrDenoiseParams), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    ),
    "pyr_session_denoised": (C.c_int, [C.c_void_p, C.POINTER(PyrDevelopParams), C.POINTER(PyrFeatureParams), C.POINTER(PyrDenoiseParams), C.c_void_p, C.c_void_p]),
    "pyr_scene_keep_previous": (C.c_int, [C.c_void_p, C.c_int]),
    "pyr_camera_world_to_cam": (C.c_int, [C.POINTER(PyrCamera), C.POINTER(C.c_float)]),
    "pyr_render_motion": (C.c_int, [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.c_void_p]),
    "pyr_render_motion_device": (C.c_int, [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrCamera), C.POINTER(PyrFilmDesc), C.c_void_p, C.c_void_p]),
    "pyr_session_motion": (C.c_int, [C.c_void_p, C.POINTER(PyrCamera), C.c_void_p]),
    "pyr_image_reproject": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrReprojectParams), C.c_void_p, C.c_void_p, C.c_int],
    ),
    "pyr_image_reproject_device": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrReprojectParams), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    ),
    "pyr_image_motion_blur": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrMotionBlurParams), C.c_void_p, C.c_int]),
    "pyr_image_motion_blur_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrMotionBlurParams), C.c_void_p, C.c_int, C.c_void_p]),
    "pyr_session_motion_blurred": (C.c_int, [C.c_void_p, C.POINTER(PyrCamera), C.POINTER(PyrDevelopParams), C.POINTER(PyrMotionBlurParams), C.c_void_p]),
    "pyr_image_temporal_resolve": (
        C.c_int,
        [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.POINTER(PyrTemporalParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    ),
    "pyr_image_temporal_resolve_device": (
        C.c_int,
        [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.POINTER(PyrTemporalParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    ),
    "pyr_image_glare": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrGlareParams), C.c_void_p, C.c_int]),
    "pyr_image_glare_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrGlareParams), C.c_void_p, C.c_int, C.c_void_p]),
    "pyr_session_glared": (C.c_int, [C.c_void_p, C.POINTER(PyrDevelopParams), C.POINTER(PyrGlareParams), C.c_void_p]),
    "pyr_image_upsample": (C.c_int, [C.c_void_p] * 3 + [C.c_uint32] * 3 + [C.c_void_p, C.c_void_p, C.POINTER(PyrUpsampleParams), C.c_void_p, C.c_int]),
    "pyr_image_upsample_device": (C.c_int, [C.c_void_p] * 3 + [C.c_uint32] * 3 + [C.c_void_p, C.c_void_p, C.POINTER(PyrUpsampleParams), C.c_void_p, C.c_int, C.c_void_p]),
    "pyr_session_upsampled": (
        C.c_int,
        [C.c_void_p, C.c_uint32, C.POINTER(PyrDevelopParams), C.POINTER(PyrFeatureParams), C.POINTER(PyrDenoiseParams), C.POINTER(PyrUpsampleParams), C.c_void_p],
    ),
    "pyr_image_despeckle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrDespeckleParams)] + [C.c_void_p] * 4 + [C.c_int]),
    "pyr_image_despeckle_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrDespeckleParams)] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    "pyr_session_despeckled": (
        C.c_int,
        [C.c_void_p, C.POINTER(PyrDevelopParams), C.POINTER(PyrDespeckleParams), C.POINTER(PyrFeatureParams), C.POINTER(PyrDenoiseParams)] + [C.c_void_p] * 4,
    ),
    "pyr_image_lens_blur": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrLensBlurParams), C.c_void_p, C.c_int]),
    "pyr_image_lens_blur_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PyrLensBlurParams), C.c_void_p, C.c_int, C.c_void_p]),
    "pyr_session_lens_blurred": (C.c_int, [C.c_void_p, C.POINTER(PyrDevelopParams), C.POINTER(PyrFeatureParams), C.POINTER(PyrLensBlurParams), C.c_void_p]),
}


def bind(lib):
    """Attach restype / argtypes for every entry point; raises AttributeError if a symbol is missing."""
    for name, (restype, argtypes) in ENTRY_POINTS.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    return lib
