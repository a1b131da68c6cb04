/*
 * goblin_hip.h -- C ABI of the MI355X-native path-tracing integrator.
 *
 * This is the drop-in boundary behind Goblin's Renderer seam.  The reference
 * has no FFI layer: the seam is the C++ virtual `Renderer::render(ScenePtr)`
 * (/root/reference/src/GoblinRenderer.h:55-59, GoblinRenderContext.h:19-22)
 * selected by `createRenderer` (GoblinContextLoader.cpp:67-92).  A GPU renderer
 * replaces that one call: scene arrays in, Film accumulation buffer out.
 *
 * Everything here is plain C: POD structs, pointers + counts, int status
 * codes, no exceptions, caller-owned output buffers.  INTEGRATION.md shows the
 * `HipPathTracer : Renderer` stub a Goblin maintainer would add on top.
 *
 * Two shared libraries implement it:
 *   libgoblin_host.so  (g++,   no HIP dependency)  gbl_host_*  scene front end
 *   libgoblin_hip.so   (hipcc, gfx950)             gbl_*       device integrator
 */
#ifndef GOBLIN_HIP_H
#define GOBLIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBL_ABI_VERSION 14

typedef enum gbl_status {
    GBL_OK = 0,
    GBL_ERR_INVALID = 1,     /* bad argument / inconsistent description       */
    GBL_ERR_UNSUPPORTED = 2, /* scene uses a Goblin feature outside the path  */
    GBL_ERR_IO = 3,          /* file missing / parse error                    */
    GBL_ERR_DEVICE = 4,      /* HIP runtime error, no device                  */
    GBL_ERR_OOM = 5,
    GBL_ERR_INTERNAL = 6     /* a C++ exception stopped at the boundary (message in *_last_error) */
} gbl_status;

/* ------------------------------------------------------------------------- */
/* Scene description (host memory, owned by the caller for the duration of    */
/* gbl_create).  Mirrors what ContextLoader builds (GoblinContextLoader.cpp   */
/* :447-504) restricted to the hot path: triangle meshes, instances,          */
/* constant-texture materials, point/spot/area lights, perspective camera.   */
/* ------------------------------------------------------------------------- */

/* position / orientation(w,x,y,z) / scale, as parsed by getTransform
 * (GoblinUtils.cpp:78-100) and composed by Transform::update
 * (GoblinTransform.cpp:182-193). */
typedef struct gbl_trs {
    float position[3];
    float orientation[4]; /* quaternion w, x, y, z */
    float scale[3];
} gbl_trs;

typedef enum gbl_shape {
    GBL_SHAPE_MESH = 0,   /* PolygonMesh, refined into triangles (GoblinPolygonMesh.cpp) */
    GBL_SHAPE_SPHERE = 1, /* Sphere(radius), intersected analytically (GoblinSphere.cpp:12-150) */
    GBL_SHAPE_DISK = 2    /* Disk(radius) in the local z = 0 plane (GoblinDisk.cpp:12-91)     */
} gbl_shape;

/* One Geometry.  A PolygonMesh after OBJ loading and (v,vn,vt) de-duplication
 * (GoblinPolygonMesh.cpp:58-262) -- vertex attributes live in the shared
 * arrays of gbl_scene_desc, indices are mesh-local -- or an analytic shape
 * (createGeometries, GoblinContextLoader.cpp:210-243), for which only
 * `shape` and `radius` are read. */
typedef struct gbl_mesh {
    uint32_t vertex_offset; /* first vertex in positions/normals/uvs          */
    uint32_t vertex_count;
    uint32_t tri_offset;    /* first triangle in indices (3 uint32 each)      */
    uint32_t tri_count;
    uint32_t has_normal;    /* PolygonMesh::hasNormal()                       */
    uint32_t has_uv;        /* PolygonMesh::hasTexCoord()                     */
    uint32_t shape;         /* gbl_shape                                      */
    float radius;           /* sphere / disk ("radius", default 1.0)          */
} gbl_mesh;

typedef enum gbl_material_type {
    GBL_MAT_LAMBERT = 0,     /* GoblinMaterial.cpp:437-480 */
    GBL_MAT_BLINN = 1,       /* GoblinMaterial.cpp:540-644 */
    GBL_MAT_TRANSPARENT = 2, /* GoblinMaterial.cpp:647-706 */
    GBL_MAT_MIRROR = 3,      /* GoblinMaterial.cpp:709-726 */
    GBL_MAT_MASK = 4,        /* GoblinMaterial.cpp:747-811: alpha-masked wrapper, BSDFnullptr punch-through */
    GBL_MAT_SUBSURFACE = 5   /* GoblinMaterial.cpp:728-745 + BSSRDF :32-220; Renderer::Lsubsurface, GoblinRenderer.cpp:128-296 */
} gbl_material_type;

typedef enum gbl_texture_type {
    GBL_TEX_CONSTANT = 0,     /* ConstantTexture,   GoblinTexture.cpp:349-354, 617-625 */
    GBL_TEX_CHECKERBOARD = 1, /* CheckboardTexture, GoblinTexture.cpp:356-416, 627-647 */
    GBL_TEX_SCALE = 2,        /* ScaleTexture,      GoblinTexture.cpp:418-425, 649-665 */
    GBL_TEX_IMAGE = 3         /* ImageTexture over a MIPMap, GoblinTexture.cpp:428-470, 40-291, 667-745 */
} gbl_texture_type;

typedef enum gbl_image_filter {   /* "filter" of an image texture (GoblinTexture.cpp:687-700); MIPMap<T>::lookup :78-97 */
    GBL_IMAGE_FILTER_NONE = 0,      /* "nearest": bilinear at level 0 (lookupNearest, :99-102) */
    GBL_IMAGE_FILTER_BILINEAR = 1,  /* one level, rounded from the footprint width (:104-110) */
    GBL_IMAGE_FILTER_TRILINEAR = 2, /* two levels blended (:112-127) */
    GBL_IMAGE_FILTER_EWA = 3        /* elliptically weighted average (:129-258) */
} gbl_image_filter;

typedef enum gbl_address_mode {   /* ImageBuffer<T>::texel, GoblinTexture.cpp:10-38 */
    GBL_ADDRESS_REPEAT = 0,
    GBL_ADDRESS_CLAMP = 1,   /* as written there: t is clamped from s (:15) */
    GBL_ADDRESS_BORDER = 2
} gbl_address_mode;

/* One MIPMap<T> (GoblinTexture.cpp:40-68): the image a texture or an image based light reads, already converted
 * (ImageTexture::convertTexel: channel pick and gamma, :489-523; the light's colour filter, GoblinLight.cpp:483-485),
 * resized to powers of two and reduced level by level with resizeImage's gaussian (:531-597).  Texels are
 * `channels` floats each (1 for float textures, 4 rgba otherwise), level 0 first, each level row-major. */
typedef struct gbl_image {
    uint32_t width, height;   /* level 0 */
    uint32_t levels;          /* floor(max(log2 w, log2 h)) + 1; level l is max(1, w >> l) x max(1, h >> l) */
    uint32_t channels;
    uint64_t texel_offset;    /* in floats, into gbl_scene_desc.texels */
} gbl_image;

typedef enum gbl_mapping_type {
    GBL_MAP_UV = 0,       /* UVMapping,        GoblinTexture.cpp:293-304 */
    GBL_MAP_SPHERICAL = 1 /* SphericalMapping, GoblinTexture.cpp:306-347 */
} gbl_mapping_type;

/* One texture of the scene's "textures" list ("format": color | float). */
typedef struct gbl_texture {
    uint32_t type;       /* gbl_texture_type                                            */
    uint32_t is_float;   /* "format" == "float"                                         */
    float value[3];      /* constant: "color", or "float" in value[0]                   */
    int32_t child[2];    /* checkerboard: texture1, texture2 (same format);
                          * scale: "texture" (same format), "scale" (float format)      */
    uint32_t mapping;    /* checkerboard: gbl_mapping_type ("mapping", default uv)      */
    float uv_scale[2];   /* uv mapping "scale" (default 1, 1)                           */
    float uv_offset[2];  /* uv mapping "offset" (default 0, 0)                          */
    gbl_trs to_tex;      /* spherical mapping: getTransform(params)                     */
    uint32_t filter;     /* checkerboard "filter" (bool, default false)                 */
    /* image textures (getImageTextureParams, GoblinTexture.cpp:677-732); mapping / uv_* / to_tex as above */
    int32_t image;          /* index into gbl_scene_desc.images, -1 otherwise                 */
    uint32_t image_filter;  /* gbl_image_filter                                                */
    uint32_t address;       /* gbl_address_mode                                                */
    float max_anisotropy;   /* "max_anisotropy" (default 10; colour image textures always use the default, :741-745) */
} gbl_texture;

/* Materials.  Each texture slot is either a constant (tex_* == -1: the value is
 * in color / color2 / exponent, createColorConstantTexture GoblinTexture.cpp:
 * 622-625) or an index into gbl_scene_desc.textures.  Colours are rgb; alpha is
 * 1 as in Color(r,g,b). */
typedef struct gbl_material {
    uint32_t type;     /* gbl_material_type                                    */
    float color[3];    /* Lambert Kd | Blinn Kg | Transparent Kr | Mirror Kr   */
    float color2[3];   /* Transparent Kt                                       */
    float index;       /* eta: blinn/transparent default 1.5, mirror 0.8       */
    float k;           /* absorption: blinn conductor iff > 0; mirror 6.0      */
    float exponent;    /* blinn exponent (float texture) | Mask alpha          */
    int32_t tex_color, tex_color2, tex_exponent; /* -1: constant above          */
    /* Mask: color = "transparent_color" (default white), exponent = "alpha"
     * (default 1), masked_material = index of the wrapped material (which must
     * not be a mask itself); -1 for every other type. */
    int32_t masked_material;
    /* Subsurface (createSubsurfaceMaterial, GoblinMaterial.cpp:881-927): color = "absorb" sigma_a, color2 =
     * "scatter_prime" sigma_s', color3 = "Kr" (default white), index = eta (default 1.5), k = "g" (default 0).  The
     * "Kd" + "mean_free_path" form is converted to sigma_a / sigma_s' by the loader exactly as the reference's
     * constructor does (BSSRDF::convertFromDiffuse, :176-212).  The material's type is BSDFAll, which carries the
     * BSDFnullptr bit: the path tracer's isOpaque / notOpaque filters treat it like a mask (GoblinPathtracer.cpp:5-11,
     * GoblinMaterial.h:393). */
    float color3[3];
    int32_t tex_color3;
    /* BumpShaders (getBumpShaders, GoblinMaterial.cpp:813-824; evaluated by Material::perturb at every closest hit,
     * GoblinScene.cpp:75-83, GoblinMaterial.cpp:221-283): "bumpmap" = a FLOAT texture displacing the surface along its
     * normal (forward differences over du = dv = 0.002), "normalmap" = a COLOUR texture holding 2 n - 1 in the shading
     * frame.  -1: none.  A mask forwards to the wrapped material's. */
    int32_t tex_bump, tex_normal;
} gbl_material;

/* InstancedPrimitive over a Model(geometry, material[, areaLight])
 * (GoblinPrimitive.cpp:99-112, GoblinModel.cpp:10-26). */
typedef struct gbl_instance {
    uint32_t mesh;
    uint32_t material;
    int32_t area_light; /* index into lights, -1 if not emissive              */
    gbl_trs to_world;
} gbl_instance;

/* Values follow Light::Type (GoblinLight.h:62-68). */
typedef enum gbl_light_type {
    GBL_LIGHT_POINT = 0,       /* GoblinLight.cpp:78-134  */
    GBL_LIGHT_DIRECTIONAL = 1, /* GoblinLight.cpp:136-210 */
    GBL_LIGHT_SPOT = 2,        /* GoblinLight.cpp:212-287 */
    GBL_LIGHT_AREA = 3,  /* GoblinLight.cpp:345-461 */
    GBL_LIGHT_IBL = 4    /* ImageBasedLight, GoblinLight.cpp:464-629 */
} gbl_light_type;

typedef struct gbl_light {
    uint32_t type;           /* gbl_light_type                                 */
    float color[3];          /* intensity (point/spot) or radiance (directional/area) */
    float position[3];       /* point/spot                                     */
    float direction[3];      /* spot/directional: as given to the light's ctor */
    float cos_theta_max;     /* spot: cos(radians(theta_max))                  */
    float cos_falloff_start; /* spot                                           */
    uint32_t mesh;           /* area: emitting geometry                        */
    gbl_trs to_world;        /* area                                           */
    uint32_t sample_num;     /* area / ibl: "sample_num" (default 1) = Light::getSamplesNum, read by the Whitted
                              * renderer's per-light quota (GoblinLight.cpp:675, GoblinWhitted.cpp:60-66); 1 for the rest */
    int32_t image;           /* ibl: the radiance map's MIPMap (already multiplied by "filter"), index into images;
                              * to_world.orientation holds "orientation" as given (the constructor's rotateX / rotateY
                              * pre-rotation is applied by gbl_create, GoblinLight.cpp:470-474) */
} gbl_light;

typedef enum gbl_camera_type {
    GBL_CAMERA_PERSPECTIVE = 0, /* GoblinCamera.cpp:83-148, 377-387 */
    GBL_CAMERA_ORTHOGRAPHIC = 1 /* GoblinCamera.cpp:288-326, 390-398 */
} gbl_camera_type;

/* PerspectiveCamera (pinhole, or thin lens when lens_radius != 0: the loader
 * then also adds the lens Disk instance, GoblinContextLoader.cpp:146-176) or
 * OrthographicCamera. */
typedef struct gbl_camera {
    float position[3];
    float orientation[4]; /* w, x, y, z */
    float fov_degrees;
    float near_plane, far_plane;
    float lens_radius, focal_distance;
    uint32_t type;        /* gbl_camera_type */
    float film_width;     /* orthographic ("film_width", default 35) */
} gbl_camera;

typedef enum gbl_filter_type {
    GBL_FILTER_BOX = 0,
    GBL_FILTER_TRIANGLE = 1,
    GBL_FILTER_GAUSSIAN = 2,
    GBL_FILTER_MITCHELL = 3
} gbl_filter_type;

/* Film + reconstruction filter (GoblinFilm.cpp:92-112,202-218,
 * GoblinFilter.h:85-106). */
typedef struct gbl_film {
    int32_t xres, yres;
    float crop[4]; /* x0 x1 y0 y1 fractions */
    uint32_t filter_type;
    float filter_width[2];
    float gaussian_falloff;
    float mitchell_b, mitchell_c;
    /* Film::writeImage post-processing (GoblinFilm.cpp:164-198, 212-215): applied by whoever develops the film --
     * gbl_film_develop on the device, or gbl_host_bloom / gbl_host_tone_map on the host; gbl_render ignores them */
    uint32_t tone_mapping;
    float bloom_radius, bloom_weight;
} gbl_film;

typedef enum gbl_integrator {
    GBL_INTEGRATOR_PATH = 0, /* PathTracer  (GoblinPathtracer.cpp) */
    GBL_INTEGRATOR_AO = 1,   /* AORenderer  (GoblinAO.cpp)         */
    /* WhittedRenderer (GoblinWhitted.cpp:13-44): emission + multiSampleLd over every light (GoblinRenderer.cpp:474-596)
     * + Lsubsurface at every level (:25-27) + the specular reflection / refraction tree (:598-648); mask materials
     * answer its requests as MaskMaterial does (GoblinMaterial.cpp:747-811).  max_ray_depth <= 12. */
    GBL_INTEGRATOR_WHITTED = 2
} gbl_integrator;

/* render_setting block (GoblinPathtracer.cpp:210-217, GoblinAO.cpp:44-49). */
typedef struct gbl_render_setting {
    uint32_t integrator;
    int32_t sample_per_pixel;
    int32_t max_ray_depth;
    int32_t bssrdf_sample_num;
    int32_t ao_sample_num;
    int32_t thread_num; /* CPU paths only */
} gbl_render_setting;

/* The scene's participating medium ("volume", GoblinContextLoader.cpp:189-207).  RenderTask::run adds it around the
 * integrator's radiance for the CAMERA ray only: sample = transmittance * Li + Lv (GoblinRenderer.cpp:40-47), the ray
 * clipped at the first surface.  Homogeneous regions only (createHomogeneousVolume, GoblinVolume.cpp:343-360);
 * "heterogeneous" (a density grid file) is GBL_ERR_UNSUPPORTED. */
typedef enum gbl_volume_type {
    GBL_VOLUME_NONE = 0,
    GBL_VOLUME_HOMOGENEOUS = 1,
    GBL_VOLUME_HETEROGENEOUS = 2   /* HeterogeneousVolumeRegion (GoblinVolume.h:106-122): sigma_t from a density grid, ray marched */
} gbl_volume_type;
typedef struct gbl_volume {
    uint32_t type;          /* gbl_volume_type                                              */
    float attenuation[3];   /* sigma_t                                                      */
    float albedo[3];        /* sigma_s = attenuation * albedo                               */
    float emission[3];
    float g;                /* Henyey-Greenstein asymmetry ("g", default 0)                 */
    int32_t sample_num;     /* light samples along the camera ray ("sample_num", default 5) */
    float box_min[3], box_max[3]; /* the region, in its own space (heterogeneous: the grid's bounding box) */
    gbl_trs to_world;
    /* GBL_VOLUME_HETEROGENEOUS (createHeterogeneousVolume, GoblinVolume.cpp:362-384): attenuation / emission unused */
    float step_size;        /* ray marching step in world units ("step_size", default 0.1)   */
    int32_t grid[3];        /* cells along x, y, z of the density grid (.vol file, float32)  */
    int32_t grid_channels;  /* 1 or 3                                                        */
    const float* density;   /* data[((z * ny + y) * nx + x) * channels + c]                  */
} gbl_volume;

typedef struct gbl_scene_desc {
    uint32_t abi_version; /* GBL_ABI_VERSION */

    uint32_t num_vertices;
    const float* positions; /* 3 per vertex */
    const float* normals;   /* 3 per vertex (zeros where the mesh has none)   */
    const float* uvs;       /* 2 per vertex (zeros where the mesh has none)   */
    uint32_t num_triangles;
    const uint32_t* indices; /* 3 per triangle, mesh-local */

    uint32_t num_meshes;
    const gbl_mesh* meshes;
    uint32_t num_materials;
    const gbl_material* materials;
    uint32_t num_textures;
    const gbl_texture* textures; /* only the non-constant ones materials reach */
    uint32_t num_images;
    const gbl_image* images;     /* MIP pyramids of image textures and image based lights */
    uint64_t num_texels;         /* floats */
    const float* texels;
    uint32_t num_instances;
    const gbl_instance* instances; /* in SceneCache::getInstances() order */
    uint32_t num_lights;
    const gbl_light* lights;       /* in SceneCache::getLights() order    */

    gbl_camera camera;
    gbl_film film;
    gbl_render_setting setting;
    gbl_volume volume;
} gbl_scene_desc;

/* ------------------------------------------------------------------------- */
/* libgoblin_host.so : scene front end (JSON + OBJ -> gbl_scene_desc).        */
/* Replaces ContextLoader::load (GoblinContextLoader.cpp:447-504) for the     */
/* subset above; same keys, defaults and int-vs-float strictness.             */
/* ------------------------------------------------------------------------- */

typedef struct gbl_host_scene gbl_host_scene;

/* Load a Goblin scene file.  Relative mesh paths resolve against the file's
 * directory (SceneCache::resolvePath, GoblinScene.cpp:236-243). */
gbl_status gbl_host_load_file(const char* json_path, gbl_host_scene** out);
/* Same, from JSON text; `scene_dir` plays the role of the file's directory. */
gbl_status gbl_host_load_string(const char* json_text, const char* scene_dir, gbl_host_scene** out);
/* The flattened description; valid until gbl_host_free. */
const gbl_scene_desc* gbl_host_desc(const gbl_host_scene* scene);
void gbl_host_free(gbl_host_scene* scene);
/* Message for the last failing gbl_host_* call on this thread. */
const char* gbl_host_last_error(void);

/* Film::getSampleRange (GoblinFilm.cpp:131-138): the film padded by the
 * filter radius.  out = {x0, x1, y0, y1}, half-open. */
void gbl_host_sample_window(const gbl_film* film, int32_t out[4]);
/* roundToSquare (GoblinUtils.h:124-130): the spp the sampler really takes. */
int32_t gbl_host_round_to_square(int32_t n);
/* Floats per Sample record when the quota depends on the scene (the Whitted renderer's per-light patterns,
 * WhittedRenderer::querySampleQuota, GoblinWhitted.cpp:46-70); equals gbl_host_sample_dimension otherwise. */
int32_t gbl_host_sample_dimension_scene(const gbl_scene_desc* desc, const gbl_render_setting* rs);
/* Floats per Sample for an integrator: 4 + quota (GoblinPathtracer.cpp:181-208,
 * GoblinAO.cpp:39-42, GoblinSampler.h:27-31). */
int32_t gbl_host_sample_dimension(const gbl_render_setting* setting);
/* Film::writeImage's normalise step (GoblinFilm.cpp:164-172): rgb/weight.
 * accum = W*H float4 {sum w*L rgb, sum w}; rgb_out = W*H*3 floats. */
void gbl_host_film_normalize(const float* accum, int32_t xres, int32_t yres, float* rgb_out);
/* Portable float map writer (build-side extra: lossless, for parity checks). */
gbl_status gbl_host_write_pfm(const char* path, const float* rgb, int32_t xres, int32_t yres);
/* Film "file" of the loaded scene, or the reference's default <scene>.exr
 * (GoblinContextLoader.cpp:127-129, 474-484).  Valid until gbl_host_free. */
const char* gbl_host_output_path(const gbl_host_scene* scene);
/* Goblin::bloom (GoblinImageIO.cpp:169-218), in place on W*H*3 floats. */
void gbl_host_bloom(float* rgb, int32_t xres, int32_t yres, float bloom_radius, float bloom_weight);
/* Goblin::toneMapping (GoblinImageIO.cpp:220-236), in place. */
void gbl_host_tone_map(float* rgb, int32_t xres, int32_t yres);
/* writeImagePPM (GoblinImageIO.cpp:101-127): ASCII P3, gamma 2.2. */
gbl_status gbl_host_write_ppm(const char* path, const float* rgb, int32_t xres, int32_t yres);
/* The same file from bytes that are already quantised (gbl_film_develop's rgb8_out): W*H*3 values, the ASCII P3 text of
 * writeImagePPM. */
gbl_status gbl_host_write_ppm8(const char* path, const uint8_t* rgb8, int32_t xres, int32_t yres);
/* writeImageEXR (GoblinImageIO.cpp:35-98): HALF channels B, G, R with tinyexr's
 * float->half rounding; scanlines are stored uncompressed (tinyexr defaults to
 * ZIP), so the pixels are the reference's, the bytes are not. */
gbl_status gbl_host_write_exr(const char* path, const float* rgb, int32_t xres, int32_t yres);
/* Goblin::writeImage (GoblinImageIO.cpp:146-167): picks the format from the
 * extension (.exr, .ppm with optional tone mapping, none/unknown -> <path>.ppm);
 * .pfm is a build-side extra.  May tone-map rgb in place. */
gbl_status gbl_host_write_image(const char* path, float* rgb, int32_t xres, int32_t yres, int32_t tone_mapping);
/* Goblin::loadImage (GoblinImageIO.cpp:14-34, 128-144): an .exr file as xres*yres float4, row-major, top row first,
 * assembled as tinyexr's LoadEXR does (one channel is replicated into all four; otherwise R, G, B must exist and A
 * defaults to 1).  Single-part scanline files, NONE / RLE / ZIPS / ZIP, HALF / FLOAT channels; anything else is
 * GBL_ERR_UNSUPPORTED, another extension GBL_ERR_IO like the reference's nullptr.  Free with gbl_host_free_image. */
gbl_status gbl_host_read_image(const char* path, float** rgba_out, int32_t* xres_out, int32_t* yres_out);
void gbl_host_free_image(float* rgba);

/* ------------------------------------------------------------------------- */
/* libgoblin_hip.so : the device integrator.                                  */
/* ------------------------------------------------------------------------- */

typedef struct gbl_ctx gbl_ctx;

typedef enum gbl_sample_mode {
    /* Counter-based device sampler with the reference's stratification law
     * (jittered strata x per-pixel sub-strata, permuted across the pixel's
     * samples: GoblinSampler.cpp:108-197), keyed by (seed, pixel, dim, k). */
    GBL_SAMPLES_NATIVE = 0,
    /* Caller uploads Sample records (device pointer): per sample
     * gbl_host_sample_dimension floats laid out {imageX, imageY, lensU1,
     * lensU2, u1D[0][..], u1D[1][..], ..., u2D[0][..], ...} exactly as
     * Sampler::requestSamples fills them; pixel-major, S samples per pixel,
     * pixels in row-major order over the sample window given in params. */
    GBL_SAMPLES_REPLAY = 1,
    /* The reference's own stream, generated on the device: one mt19937 per 8x8
     * sample tile (RNGImp, GoblinUtils.cpp:13-56) seeded with the tile's value
     * of the never-seeded libc rand() in row-major tile order (RenderTask,
     * GoblinRenderer.cpp:29-52, 99-126), Sampler::requestSamples per pixel
     * (GoblinSampler.cpp:108-197) and the three discarded floats of every
     * BSDFSample(rng) in PathTracer::Li (GoblinPathtracer.cpp:103,150,159).
     * A participating medium's draws follow each sample's Li draws in the
     * tile's stream (RenderTask::run, GoblinRenderer.cpp:43-46): carried too.
     * The Film accumulators then equal the reference binary's (glibc /
     * libstdc++ build) up to float summation order, with nothing uploaded.
     * A tile is sequential by construction -- this is the bit-faithful mode,
     * NATIVE the fast one.  All three integrators, megakernel schedule only;
     * the window must be whole tiles of the full sample window. */
    GBL_SAMPLES_STREAM = 2
} gbl_sample_mode;

/* How the device schedules the same arithmetic (identical per-sample radiance):
 *  WAVEFRONT   path pool in HBM, compacted ray queues, extend / shade / shadow kernels
 *  MEGAKERNEL  one persistent kernel, path state in registers, in-wave regeneration */
/* AUTO (path tracer): WAVEFRONT when the scene's paths are long -- at least RAYS_PER_PATH scene queries per camera path, measured
 * once per context and max_ray_depth by a one-sample pilot inside the first such gbl_render call (which therefore synchronises)
 * -- and the call (this rank's tiles x spp) holds at least PATHS camera samples; MEGAKERNEL otherwise and for mask scenes, AO,
 * Whitted and GBL_SAMPLES_STREAM (gbl_stats.schedule reports what a call ran under) */
#define GBL_AUTO_WAVEFRONT_RAYS_PER_PATH 6.0f
#define GBL_AUTO_WAVEFRONT_PATHS (1ull << 22)
typedef enum gbl_schedule {
    GBL_SCHEDULE_AUTO = 0,
    GBL_SCHEDULE_MEGAKERNEL = 1,
    GBL_SCHEDULE_WAVEFRONT = 2
} gbl_schedule;

typedef struct gbl_render_params {
    uint32_t integrator;      /* gbl_integrator                               */
    int32_t sample_per_pixel; /* rounded up to a square like the reference    */
    int32_t max_ray_depth;    /* PathTracer: loop runs max_ray_depth-1 times  */
    int32_t ao_sample_num;
    int32_t bssrdf_sample_num; /* only sizes the replay record (dims)         */
    /* sub-window of the sample window to render, half-open pixel coords; the
     * multi-GPU shard unit.  {0,0,0,0} = the whole Film::getSampleRange. */
    int32_t window[4];        /* x0, x1, y0, y1 */
    /* Interleaved tile sharding inside the window: this call renders only the
     * 8x8-pixel sample tiles t (row-major over the window) with
     * t % tile_shard_count == tile_shard_index.  count <= 1 renders every tile.
     * One GPU per shard + gbl_film_allreduce reproduces the whole film. */
    int32_t tile_shard_index;
    int32_t tile_shard_count;
    uint32_t sample_mode;     /* gbl_sample_mode                              */
    uint64_t seed;            /* native mode                                  */
    const float* replay_samples; /* device pointer, replay mode               */
    /* optional device pointer: per-sample radiance rgba as Li() returns it,
     * same order as the samples (replay/native), or NULL. */
    float* li_out;
    uint32_t russian_roulette; /* build-side extension; MUST be 0 for parity
                                  (the reference loop is fixed length,
                                  GoblinPathtracer.cpp:76)                    */
    uint32_t collect_stats;    /* fill node/triangle counters (slower)        */
    uint32_t schedule;         /* gbl_schedule                                */
    uint32_t exact_ties;       /* native sampler, scenes of the headline feature set (the lean kernels): follow the reference's
                                  BVH where two triangles are accepted at exactly the same t, and its non-watertight box tests
                                  where a ray grazes one.  Every other render does anyway (replay, stream,
                                  instrumented, scenes that need the EXT kernels); here it costs ~16 % for the few rays per
                                  10^6 it decides, so it is off by default                                              */
    void* stream;              /* hipStream_t, NULL = default stream          */
} gbl_render_params;

typedef struct gbl_stats {
    uint64_t paths;          /* camera samples = Li evaluations               */
    uint64_t extension_rays; /* closest-hit scene queries (incl. primary)     */
    uint64_t shadow_rays;    /* any-hit scene queries                         */
    uint64_t nodes;          /* child boxes tested (32 B each)                */
    uint64_t tris;           /* triangles tested (48 B each)                  */
    uint64_t splats;         /* film pixel updates                            */
    uint64_t dims;           /* sample dimensions consumed (floats)           */
    double kernel_ms;        /* HIP-event time of the render kernel(s)        */
    uint32_t schedule;       /* the gbl_schedule the call ran under (what GBL_SCHEDULE_AUTO resolved to; megakernel for AO / Whitted) */
    uint32_t reserved;
} gbl_stats;

/* Build the two-level BVH on the host, pack and upload the scene once
 * (replaces Scene/BVH/Model construction: GoblinScene.cpp:11-27,
 * GoblinBVH.cpp:34-151, GoblinModel.cpp:10-26).  `device` is a HIP ordinal. */
gbl_status gbl_create(const gbl_scene_desc* desc, int device, gbl_ctx** out);
/* Same with flags (GBL_CREATE_*, declared below).  gbl_create is gbl_create_ex
 * with flags 0, or GBL_CREATE_DEVICE_BVH when GBL_BVH_BUILD=device is set. */
gbl_status gbl_create_ex(const gbl_scene_desc* desc, int device, uint32_t flags, gbl_ctx** out);

/* Run the integrator over params->window and ACCUMULATE into film_accum, a
 * device buffer of xres*yres float4 {sum w*L.rgb, sum w} (the per-thread
 * ImageTile of the reference, GoblinFilm.cpp:61-90).  Replaces
 * Renderer::render's task loop (GoblinRenderer.cpp:99-126, 29-52).
 * Asynchronous on params->stream unless stats != NULL (then it synchronises
 * to read counters and timing). */
gbl_status gbl_render(gbl_ctx* ctx, const gbl_render_params* params, float* film_accum, gbl_stats* stats);

/* Sum film_accum across the ranks of an RCCL communicator (ncclComm_t passed
 * as void*): replaces Film::mergeTile under the TLS mutex
 * (GoblinFilm.cpp:140-153, GoblinThreadLocalStorage.h:69-75). */
gbl_status gbl_film_allreduce(gbl_ctx* ctx, void* rccl_comm, float* film_accum, void* stream);

/* Device-side Film::writeImage normalise: rgb_out[W*H*3] = rgb / weight. */
gbl_status gbl_film_resolve(gbl_ctx* ctx, const float* film_accum, float* rgb_out, void* stream);

typedef struct gbl_develop_params {
    float bloom_radius, bloom_weight; /* either <= 0: no bloom (GoblinFilm.cpp:188) */
    uint32_t tone_mapping;            /* Goblin::toneMapping before the outputs are written */
    uint32_t reserved;
    void* stream;                     /* hipStream_t, NULL = default stream */
} gbl_develop_params;

/* Film::writeImage's tail on the device: rgb = accum.rgb * (1 / accum.w) exactly as gbl_film_resolve,
 * then Goblin::bloom, then (tone_mapping) Goblin::toneMapping.  rgb_out: W*H*3 floats, or NULL.
 * rgb8_out: W*H*3 bytes = writeImagePPM's int(clamp(powf(c, 1/2.2f), 0, 1) * 255), or NULL.
 * Asynchronous on params->stream; scratch lives in the context.
 * Both are device pointers; one of them may be NULL, rgb_out may not alias film_accum.  The pixels are the reference's bit
 * for bit (glibc's powf / logf / expf restated for the device, the reference's order in every sum).  The scratch and the
 * cached bloom filter table belong to the context: calls that share a context are ordered by the caller, on one stream or
 * by events.  Pixels of weight 0 and negative or non-finite values are unspecified, as for gbl_host_write_ppm. */
gbl_status gbl_film_develop(gbl_ctx* ctx, const float* film_accum, const gbl_develop_params* params,
                            float* rgb_out, uint8_t* rgb8_out);

/* First-hit features of the camera samples.  Camera sample i is the one gbl_render draws for the same
 * params (sample_mode, seed, sample_per_pixel, window, tile shard, and the integrator / depth fields that size a replay
 * record): record i here and entry i of li_out describe the same camera ray.  The ray is traced as Scene::intersect does it --
 * unfiltered closest hit, mint from the camera, Material::perturb on the fragment (GoblinScene.cpp:75-83); exact_ties as in
 * gbl_render.  A miss leaves hit = 0, t = -1, instance = -1 and zeros. */
typedef struct gbl_aov_sample {      /* 48 bytes */
    float albedo[3];   /* the material's first colour slot as the bounce-0 BSDF reads it: Lambert Kd, Blinn Kg, transparent /
                        * mirror Kr (color / tex_color), subsurface Kr (color3 / tex_color3), a mask's wrapped material's;
                        * texture lookups see the camera ray's differentials (computeUVDifferential, GoblinPathtracer.cpp:77) */
    float t;           /* the ray parameter of the hit (ray.maxt after the query) */
    float normal[3];   /* world-space shading normal after perturb, NOT flipped towards the viewer */
    int32_t instance;  /* index into gbl_scene_desc.instances */
    float position[3]; /* the fragment's world position */
    uint32_t hit;
} gbl_aov_sample;
typedef struct gbl_aov_targets {     /* device pointers; any may be NULL, not all */
    /* films of xres*yres float4, ACCUMULATED into through the reconstruction filter like gbl_render's; a sample whose
     * feature is NaN is dropped from that film (ImageTile::addSample's rule, GoblinFilm.cpp:62-66) */
    float* albedo_accum;   /* {sum w*albedo.rgb, sum w}; a miss contributes 0 with its weight */
    float* normal_accum;   /* {sum w*n.xyz, sum w} */
    float* depth_accum;    /* {sum w*t*hit, sum w*hit, 0, sum w}: depth = x / y, coverage (alpha) = y / w */
    gbl_aov_sample* samples_out;     /* one per camera sample of the call, li_out's order */
} gbl_aov_targets;
/* Asynchronous on params->stream unless stats != NULL; stats reports paths, extension_rays = paths, kernel_ms and, under
 * collect_stats, the node / triangle counters.  li_out, russian_roulette and schedule are ignored; the medium, the lights and
 * max_ray_depth do not enter.  GBL_SAMPLES_STREAM is GBL_ERR_UNSUPPORTED (that stream's image positions depend on the draws Li
 * makes).  Internal memory is a chunk of samples per pixel at a time, inside gbl_render's per-sample budget.  The films are
 * ordinary accumulators: gbl_film_allreduce reduces them, gbl_film_resolve normalises the first two. */
gbl_status gbl_render_aov(gbl_ctx* ctx, const gbl_render_params* params, const gbl_aov_targets* targets, gbl_stats* stats /* or NULL */);
/* depth_out[W*H] = x / y (IEEE divide) and coverage_out[W*H] (or NULL) = y / w of depth_accum; 0 where the denominator is 0. */
gbl_status gbl_aov_resolve_depth(gbl_ctx* ctx, const float* depth_accum, float* depth_out, float* coverage_out, void* stream);

/* Variance of the pixel mean from per-sample radiance.  li: n x 4 floats in gbl_render's li_out order --
 * pixel-major over `window`, S entries per pixel; window and sample_per_pixel as in gbl_render_params ({0,0,0,0} or NULL =
 * the whole sample window, S rounded up to a square).  For every window pixel inside the image, with
 * l_k = (0.2126f r + 0.7152f g) + 0.0722f b of sample k and the samples whose l_k is not finite dropped (ImageTile::addSample's
 * rule), m samples left:  mean = (sum l) / m,  variance_out[y * xres + x] = (sum (l - mean)^2) / (m (m - 1)) in float32, m (m - 1)
 * formed in float32; 0 when m < 2.  Both sums run over k = 0 .. S-1 in that order, one after the other, so the plane is
 * reproducible bit for bit.  Window pixels outside the image (the filter border) are ignored; image pixels outside the window
 * are not written.  S < 2 is GBL_ERR_INVALID.  Under a tile shard the li entries of tiles the call does not own are zero, so
 * their variance is 0: the planes of disjoint shards add up to the whole plane under gbl_film_allreduce-style summation.
 * Asynchronous on `stream`. */
gbl_status gbl_film_variance(gbl_ctx* ctx, const float* li, const int32_t window[4], int32_t sample_per_pixel,
                             float* variance_out /* xres*yres */, void* stream);

/* Edge-avoiding a-trous wavelet filter of a film, guided by the first-hit films of gbl_render_aov and by the variance of the
 * pixel mean (DESIGN.md 4.6 states the filter operation by operation).  All inputs are complete films (with several GPUs:
 * after gbl_film_allreduce); each guide may be NULL and its term then drops out.  Without depth_accum every pixel counts as
 * covered.  film_out: xres*yres float4, {rgb, 1} for a valid pixel and {0,0,0,0} for an invalid one (weight 0 or a
 * non-finite input), so gbl_film_resolve and gbl_film_develop take it unchanged; it may not overlap an input.  An invalid pixel
 * neither contributes to nor receives from a neighbour.  A pixel whose neighbours all weigh 0 keeps its colour to within one
 * rounding of (h c) / h.  Asynchronous on params->stream; the scratch (four float4 planes) lives in the context: calls that
 * share a context are ordered by the caller. */
typedef struct gbl_denoise_params {
    int32_t iterations;                 /* 1..8 a-trous levels; level i taps at stride 2^i */
    float sigma_luminance;              /* > 0; in standard deviations of the pixel mean when a variance plane is given */
    float sigma_normal, sigma_albedo, sigma_depth;   /* > 0, each read only if its film is given */
    uint32_t demodulate;                /* divide by albedo before filtering, multiply back after; needs albedo_accum */
    void* stream;                       /* hipStream_t, NULL = default stream */
} gbl_denoise_params;
gbl_status gbl_film_denoise(gbl_ctx* ctx, const float* film_accum, const float* variance /* or NULL */,
                            const float* albedo_accum, const float* normal_accum, const float* depth_accum /* each or NULL */,
                            const gbl_denoise_params* params, float* film_out /* xres*yres float4 */);

/* Reprojected temporal accumulation of a film (DESIGN.md 4.7 states it operation by operation): the frame just rendered is
 * blended into a history fetched from where each pixel's surface point lay under the previous camera, with a history length per
 * pixel.  The current camera is the context's (gbl_update_camera); the history is the caller's, so a context holds no frame
 * state and a caller may keep several.  A history is three planes of xres*yres float4 in device memory, one after the other:
 * H0 = {c.rgb, N}, H1 = {m1, m2, v, z}, H2 = {n.xyz, surf ? 1 : 0} -- accumulated colour and history length, the first two
 * moments of the luminance, the variance of the accumulated pixel, and the depth and normal the next frame tests its taps
 * against.  history_in = NULL starts a sequence (N = 1 everywhere).  history_out may not overlap history_in: the gather reads
 * neighbours.  film_out: {rgb, 1} for a valid pixel, zeros (in every output, so N = 0) for one of weight 0 or with a non-finite
 * input; it takes the denoiser's place in the chain, and gbl_film_denoise(film_out, variance_out, albedo, normal, depth),
 * gbl_film_resolve and gbl_film_develop accept it unchanged.  variance_out is the variance of the accumulated pixel: blended
 * from `variance` where that plane is given, otherwise estimated from the accumulated luminance moments (N >= 4) or from the
 * 5 x 5 neighbourhood of the current frame -- a variance for films that arrive without per-sample radiance.  Limits: a thin
 * lens is reprojected as its pinhole; pixels without coverage (the background) do not accumulate; moving instances are not
 * reprojected here, a moved instance ghosts until the depth or normal test rejects it: gbl_render_motion and
 * gbl_film_accumulate_motion below carry them.  No output may overlap an input or another output.  Asynchronous on params->stream; the scratch lives in the context: calls that share a context are ordered by the
 * caller. */
#define GBL_HISTORY_FLOATS_PER_PIXEL 12   /* three float4 planes of xres*yres, caller-owned, device memory */
typedef struct gbl_temporal_params {
    gbl_camera prev_camera;  /* the camera history_in was accumulated under; ignored when history_in is NULL */
    float alpha_min;         /* in (0, 1]: floor of the blend weight */
    float max_history;       /* >= 1: the history length is clamped to it */
    float sigma_depth;       /* > 0: relative depth tolerance of a history tap and of the spatial estimate */
    float cos_normal;        /* in [-1, 1]: smallest n_prev . n_cur of an accepted tap; read only with a normal film */
    uint32_t reserved;
    void* stream;            /* hipStream_t, NULL = default stream */
} gbl_temporal_params;
gbl_status gbl_film_accumulate(gbl_ctx* ctx, const float* film_accum, const float* variance /* or NULL */,
                               const float* normal_accum /* or NULL */, const float* depth_accum,
                               const float* history_in /* or NULL: first frame */, float* history_out,
                               const gbl_temporal_params* params, float* film_out /* float4, {rgb, 1} */,
                               float* variance_out /* xres*yres, or NULL */);

/* Motion planes: per image pixel, where the surface point under the pixel's centre lay in the previous frame --
 * under params->prev_camera and, for an instance whose transform changed since, under its previous transform.  The ray is the
 * context camera's through (x + 0.5, y + 0.5), pinhole or orthographic (a thin lens counts as its pinhole), traced as
 * gbl_render_aov traces a camera ray without exact_ties.  On a hit of instance i at P: P_prev = M_prev[i] (Minv_cur[i] P) if the
 * instance moved, else P itself, projected through prev_camera exactly as gbl_film_accumulate projects its point.
 * motion_out is two planes of xres*yres float4 in device memory, one after the other:
 *   M0 = {image_x, image_y, z_exp, ok}   ok = 1 iff the ray hit, P_prev lies in front of prev_camera and all three are finite;
 *                                        otherwise the texel is all zeros
 *   M1 = {n_b.xyz, instance + 1}         0 in .w on a miss.  n_b: the current frame's normal (normal_accum resolved as
 *                                        gbl_film_accumulate resolves it; zeros without one) carried into the previous frame by
 *                                        the inverse transpose of the same pair of transforms, unit length or 0; n itself for an
 *                                        unmoved instance and on a miss
 * prev_to_world: one gbl_trs per instance of the context (what gbl_get_instances returned when the previous frame was
 * rendered), or NULL: no instance moved.  An instance moved iff its ten floats differ bitwise from the current ones, so a static
 * scene is reprojected without a round trip through two matrices.  GBL_ERR_INVALID: a NULL params or motion_out, motion_out
 * overlapping normal_accum, an unknown prev_camera.type, a non-finite previous transform and one the reference cannot invert
 * (|det| < 1e-5, as gbl_create refuses it); GBL_ERR_UNSUPPORTED: 2^24 - 1 or more instances (the id must be exact in a float).
 * Always the whole image: no window, no shard -- the planes are not accumulators, so with several GPUs every rank computes
 * them.  Asynchronous on params->stream (the table of previous transforms is uploaded from pageable memory when an instance
 * moved); that table lives in the context: calls that share a context are ordered by the caller. */
#define GBL_MOTION_FLOATS_PER_PIXEL 8   /* two float4 planes of xres*yres, caller-owned, device memory */
typedef struct gbl_motion_params {
    gbl_camera prev_camera;        /* the camera of the previous frame */
    const gbl_trs* prev_to_world;  /* host, one per instance, or NULL: no instance moved */
    const float* normal_accum;     /* device, the current frame's normal film, or NULL */
    void* stream;                  /* hipStream_t, NULL = default stream */
} gbl_motion_params;
gbl_status gbl_render_motion(gbl_ctx* ctx, const gbl_motion_params* params, float* motion_out);

/* gbl_render_motion for meshes whose vertices were edited since the previous frame (gbl_update_vertices): the same ray, query,
 * miss handling, planes and refusals, and the previous pose of every mesh in prev_meshes.  A listed mesh is DEFORMED iff its
 * previous positions differ bitwise from the ones the context holds (gbl_get_vertices); a listed but unchanged mesh, an unlisted
 * one, a sphere and a disk take gbl_render_motion's path, so with num_prev_meshes == 0 or every listed mesh unchanged the planes
 * are gbl_render_motion's bit for bit.  On a hit of instance i of a deformed mesh, in triangle T at barycentrics (b1, b2):
 *   Q = (v0' + (v1' - v0') b1) + (v2' - v0') b2      T's vertices in the previous pose, object space
 *   P_prev = M Q                                      M: the instance's previous transform if it moved, else its current one
 * projected as gbl_render_motion projects its point; M1.w = i + 1 as there.  With a normal film, n_b is the film's normal carried
 * by the inverse transpose of the map that takes T's current edges and unit normal to the previous ones (to object space by the
 * instance's current transform first, on to the previous frame's world by M afterwards), unit length or 0; a triangle without
 * area in either pose carries it by the instance's transforms alone.
 * Limits: only the first hit is followed -- shadows, reflections and refractions of a deforming surface are not tracked; a map
 * that perturbs the shading normal is carried as the film's normal by the geometric deformation.
 * GBL_ERR_INVALID, before the context is touched: everything gbl_render_motion refuses, a NULL prev_meshes with
 * num_prev_meshes > 0, a NULL positions, a mesh index out of range or a mesh that is a sphere or a disk, a mesh listed twice,
 * reserved != 0 and a non-finite coordinate.  The previous positions of the deformed meshes are copied to a table of the context
 * and uploaded on params->stream, as the previous transforms are; the caller's arrays are not read after the call returns. */
typedef struct gbl_motion_mesh {
    uint32_t mesh;            /* gbl_scene_desc::meshes index of a triangle mesh */
    uint32_t reserved;        /* 0 */
    const float* positions;   /* host, 3 * vertex_count: gbl_get_vertices(mesh) as it was when the previous frame was rendered */
} gbl_motion_mesh;
gbl_status gbl_render_motion_deform(gbl_ctx* ctx, const gbl_motion_params* params, const gbl_motion_mesh* prev_meshes,
                                    uint32_t num_prev_meshes, float* motion_out);
/* gbl_render_motion_deform with every gbl_motion_mesh::positions pointing to DEVICE memory (gbl_get_vertices_device before the
 * edit): the same planes bit for bit, the same refusals in the same order, and for each positions pointer the two pointer
 * refusals of gbl_update_vertices_device.  Finiteness is checked by a kernel, and which listed meshes are deformed is decided by
 * another, bitwise against the positions the device holds; one word per listed mesh is read back for each, behind a wait for
 * params->stream (the choice of kernel depends on the answer).  The deformed meshes' previous positions are copied device to
 * device into the context's table on params->stream; whatever writes the caller's arrays next must be ordered behind that
 * stream.  No tie order is made (see gbl_update_vertices_device): none of gbl_render_motion's kernels reads it. */
gbl_status gbl_render_motion_deform_device(gbl_ctx* ctx, const gbl_motion_params* params, const gbl_motion_mesh* prev_meshes /* .positions: device */,
                                           uint32_t num_prev_meshes, float* motion_out);

/* gbl_film_accumulate with the reprojection read from `motion` (gbl_render_motion's planes for this frame) instead of
 * computed from the depth film and params->prev_camera, which is not read: (image_x, image_y, z_exp) = M0.xyz, a pixel with
 * M0.w == 0 has no history, and with a normal film the taps are tested against M1.xyz in place of n (H2 still stores n).
 * Everything else is gbl_film_accumulate's, word for word: prepare, the four taps and their order, blend, both variance
 * paths, outputs and refusals, to which a NULL `motion` and one overlapping an output are added.  The history planes keep their
 * layout, so a history may pass between the two calls.  Limits: taps are not rejected by instance id (M1.w is for the caller);
 * the depth a tap is tested against is the centre ray's, not the filtered film's. */
gbl_status gbl_film_accumulate_motion(gbl_ctx* ctx, const float* film_accum, const float* variance /* or NULL */,
                                      const float* normal_accum /* or NULL */, const float* depth_accum,
                                      const float* history_in /* or NULL: first frame */, float* history_out,
                                      const float* motion /* gbl_render_motion's planes */, const gbl_temporal_params* params,
                                      float* film_out /* float4, {rgb, 1} */, float* variance_out /* xres*yres, or NULL */);

/* Device time of recent gbl_render calls, from HIP events recorded on the render stream
 * around the dominant kernel and around the whole call (no host synchronisation happens
 * inside gbl_render for this).  out[0] is the most recent call.  Blocks until those events
 * have completed.  Returns the number of entries filled (at most 64 calls are remembered). */
typedef struct gbl_timing {
    double main_kernel_ms; /* path_trace_kernel / ao_kernel (megakernel schedule) or all
                              wf_* kernels of the call (wavefront schedule)            */
    double total_ms;       /* main kernel(s) + film splat kernel                        */
} gbl_timing;
int gbl_get_timings(gbl_ctx* ctx, int n, gbl_timing* out);

/* Scene facts the caller needs for buffer sizing and reporting. */
/* gbl_create_ex flags */
#define GBL_CREATE_DEVICE_BVH 1u /* build the triangle BLASes on the GPU (Morton-sorted linear BVH) instead of the
                                  * host's binned-SAH build: faster to construct, slower to trace */

typedef struct gbl_info {
    int32_t xres, yres;
    int32_t window[4];      /* full sample window x0,x1,y0,y1 */
    uint64_t blas_nodes, tlas_nodes, triangles, instances;
    uint64_t scene_bytes;   /* device bytes held by the scene */
    uint64_t instanced_triangles; /* sum over instances of their mesh's triangle count */
    double build_ms;        /* host wall time of scene packing + BVH build + geometry upload in gbl_create */
    int32_t blas_depth, tlas_depth; /* 4-wide levels */
} gbl_info;
gbl_status gbl_get_info(const gbl_ctx* ctx, gbl_info* out);

/* Instance edits: give instances [first, first + count) new transforms and rebuild the TLAS over all instances in
 * place (BLASes untouched; the reference would rebuild its whole scene BVH, GoblinScene.cpp:11-27).  Synchronises
 * the device.  Instances that carry an area light, and scenes with a directional or image based light (whose power and
 * sampling sphere depend on the scene bound), are GBL_ERR_UNSUPPORTED: re-create the context for those. */
gbl_status gbl_update_instances(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* to_world);
/* The transforms the context holds now for instances [first, first + count): gbl_create's at first, the edited ones after
 * gbl_update_instances.  Host only.  What a caller keeps, next to the camera, as "the previous frame" for gbl_render_motion: the
 * context holds no frame state.  GBL_ERR_INVALID for a NULL argument or a range out of bounds. */
gbl_status gbl_get_instances(const gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_trs* out);

/* gbl_update_instances with the transforms read from DEVICE memory: what a rigid-body or particle step on the GPU leaves behind
 * goes into the context without a trip through the host.  d_to_world holds `count` gbl_trs records of 40 bytes.
 *  - flags == 0: after the call every device table -- the instance records and bounds, the TLAS's used records, and gbl_info --
 *    is byte for byte what gbl_update_instances leaves when fed the same floats.  Order of the call: synchronise; one kernel
 *    composes the edited instances' m / inv and world boxes into staging and folds refusals into a word; 8 bytes are read back;
 *    the instance bounds are read back and the TLAS is built on the host as in every edit; upload and commit; synchronise.
 *  - GBL_INSTANCES_DEVICE_TLAS: the TLAS is built on the device over the instance bounds by the linear builder
 *    (gbl_create_ex's GBL_CREATE_DEVICE_BVH builder, a leaf being one instance) and lands in the TLAS's reserved node records.
 *    What crosses the bus: the refusal word, 8 bytes of counters per level of the tree, and the tree's used records (64 bytes
 *    per node, at most one per instance), which the exact traversal-stack rule is evaluated over.  A render under the tie rule
 *    (exact_ties, replay, stream, instrumented, Whitted, every EXT build) equals, bit for bit, that of a fresh context of the
 *    edited scene; the linear tree is faster to build and slower to trace than the host's.  Any later host-tail edit
 *    (gbl_update_instances, gbl_update_vertices*, gbl_rebuild_mesh) puts a host-built TLAS back.  A context with fewer than
 *    two instances ignores the flag.
 *  - The context's host copy of the transforms becomes a mirror: the edit marks its range stale, and gbl_get_instances,
 *    gbl_update_instances, the geometry edits and gbl_render_motion* refresh it with one download of the stale range when they
 *    need it.  The raw transforms are kept in a device table made at the first call of this entry or of
 *    gbl_get_instances_device and written by every instance edit after that.
 * Refusals, the context untouched: GBL_ERR_INVALID for a NULL pointer, unknown bits in flags, a pointer that is not device or
 * managed memory of the context's device, an allocation that ends before 40 * count bytes; gbl_update_instances' own with its
 * messages (range out of bounds, a directional or image based light, an instance that carries an area light); then, met by the
 * kernel: GBL_ERR_INVALID for a transform with a float that is not finite (the host entry does not check this), naming the lowest
 * such instance, and, when no transform is non-finite, gbl_update_instances' |det| < 1e-5 refusal for the lowest such instance.
 * With GBL_INSTANCES_DEVICE_TLAS also GBL_ERR_INVALID for a world bound that overflows a float.  count == 0 with a valid
 * pointer is GBL_OK and changes nothing. */
#define GBL_INSTANCES_DEVICE_TLAS 1u
gbl_status gbl_update_instances_device(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* d_to_world /* device, count records of 40 B */,
                                       uint32_t flags);
/* gbl_get_instances into DEVICE memory: a device-to-device copy from the context's raw transform table, complete when the call
 * returns.  Before any device edit the table is uploaded from the host's values.  GBL_ERR_INVALID for a NULL argument, a range
 * out of bounds and the pointer refusals above. */
gbl_status gbl_get_instances_device(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_trs* d_out /* device */);
/* Self-test hook: the DevInstance records (128 B: m[12], inv[12], root, material, area_light, mesh, shape, radius, is_mask, pad)
 * and the DevInstanceBound records (24 B: lo[3], hi[3]) of instances [first, first + count) to host memory, and *total (the
 * instance count), *tlas_root and *stack_entries as the context holds them now.  Any out pointer may be NULL.  Synchronises the
 * device when it copies. */
gbl_status gbl_selftest_instances(gbl_ctx* ctx, uint64_t first, uint64_t count, void* records_out, void* bounds_out, uint64_t* total, int32_t* tlas_root,
                                  int32_t* stack_entries);

/* Vertex edit: give vertices [first, first + count) of triangle mesh `mesh` (gbl_scene_desc::meshes index; vertex numbers are the
 * mesh's own, 0 .. vertex_count) new object-space positions, and new normals if `normals` is not NULL.  The mesh's BLAS is
 * refitted on the device in place; nothing is rebuilt on the host but the TLAS.
 *  - The topology is kept: indices, triangle count, the tree's shape, the leaves' contents and every reference.  Only values
 *    derived from positions are computed again: the triangles' p0 / e1 / e2 and bounds, the nodes' quantised child boxes, the
 *    reference's visiting order (what exact ties are broken by), the mesh's object bound, the instance bounds and the TLAS.
 *  - After the call every table the kernels read is what it would be for the edited positions over the same tree, and a render
 *    equals, bit for bit, that of a context created from the edited scene.  A tree refitted after a large deformation is valid
 *    but slower to trace than a new one: gbl_mesh_tree_stats measures it and gbl_rebuild_mesh builds it again in place.
 *  - The call synchronises the device, as gbl_update_instances does, and GBL_SCHEDULE_AUTO measures its rays per path again.
 *  - normals == NULL: the mesh's vertex normals stay as they were.  The caller owns that choice.
 *  - gbl_render_motion's planes follow cameras and instances only; gbl_render_motion_deform also takes the positions a mesh had
 *    in the previous frame (gbl_get_vertices before the edit) and follows the deformation of the surface under each pixel.
 * GBL_ERR_INVALID, the context untouched: a NULL ctx or positions, a mesh index out of range or a mesh that is a sphere or a
 * disk, a vertex range out of bounds, a non-finite coordinate, normals given for a mesh without has_normal.
 * GBL_ERR_UNSUPPORTED, the context untouched: a mesh an area light emits from (its emitting triangles, area distribution and
 * power would have to follow), and scenes with a directional or image based light, whose power and sampling sphere depend on
 * the scene bound -- what gbl_update_instances refuses for the same reason.  (A participating medium needs no refusal: the
 * scene bound it carries is read by those two kinds of light only.)  positions and normals are host pointers. */
gbl_status gbl_update_vertices(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count,
                               const float* positions /* host, 3 * count */, const float* normals /* host, 3 * count, or NULL */);
/* The positions the context holds now (gbl_create's at first).  Host only, like gbl_get_instances, but for the first call after a
 * gbl_update_vertices_device of the mesh, which downloads the mesh's positions once.  GBL_ERR_INVALID for a NULL argument, a mesh
 * out of range or not a triangle mesh, a range out of bounds. */
gbl_status gbl_get_vertices(const gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, float* positions_out);

/* gbl_update_vertices with positions and normals read from DEVICE memory: what a skinning or morphing step on the GPU leaves
 * behind goes into the context without a trip through the host.  After the call every device table -- nodes, triangles, their
 * bounds, positions, normals, instance records and bounds, the TLAS, and the tie order unless deferred -- is byte for byte what
 * gbl_update_vertices leaves when fed the same floats.
 *  - Order of the call: synchronise; the finiteness check (a kernel; 4 bytes read back); the refit plan on the mesh's first edit;
 *    device-to-device copies; gbl_update_vertices' refit launches; the mesh's object bound on the device (24 bytes read back); the
 *    TLAS on the host as in every edit; synchronise.  Nothing else crosses the bus.
 *  - The context's host copy of the positions becomes a mirror: the edit marks the mesh's slice stale, and gbl_get_vertices,
 *    gbl_update_vertices, gbl_render_motion_deform and the tie order refresh it with one download of the slice when they need it.
 *  - The tie order (the reference's visiting order, what exact ties are broken by) is made on the host from the mirror, as
 *    gbl_update_vertices makes it: about 7.6 ms for the bunny's 69 451 triangles, beside 0.2 ms for everything else.  Only the
 *    kernels compiled with the tie rule read it: replay, stream, instrumented and exact_ties renders, Whitted, and every kernel of
 *    a scene beyond the headline feature set (the EXT builds).  With GBL_VERTICES_DEFER_ORDER the mesh is marked pending instead
 *    (gbl_order_pending), and the first call that launches such a kernel -- gbl_render, gbl_render_aov, gbl_selftest_trace -- or
 *    reads the table (gbl_selftest_geometry table 3), or a gbl_update_vertices of the mesh, makes the order of every pending
 *    mesh before it queues anything (one more synchronisation).  A call that launches lean kernels only -- gbl_render under the
 *    native sampler without exact_ties and collect_stats, gbl_render_aov likewise, every gbl_render_motion* -- leaves it pending
 *    and never pays for it.  (GBL_SCHEDULE_AUTO's pilot after an edit is an instrumented render: it makes the order.)
 *    What deferral buys: a frame loop on a lean scene edits in 0.2 ms instead of 7.8.  What it does not: the cost is moved, not
 *    removed -- a scene that needs the EXT kernels pays the same 7.6 ms inside its next render.
 * Refusals, the context untouched: gbl_update_vertices' own with its messages (the host-side ones first; a non-finite coordinate
 * is met last, by the kernel, with the host entry's message: the lowest float index decides, a position before a normal), and
 * GBL_ERR_INVALID for unknown bits in flags, for a pointer that is not device or managed memory of the context's device (a
 * plain host pointer is refused before anything reads it), and for one whose allocation ends before 12 * count bytes. */
#define GBL_VERTICES_DEFER_ORDER 1u
gbl_status gbl_update_vertices_device(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, const float* d_positions /* device, 3 * count */,
                                      const float* d_normals /* device, 3 * count, or NULL */, uint32_t flags);
/* gbl_get_vertices into DEVICE memory: a device-to-device copy of the positions the context holds now, complete when the call
 * returns.  What a frame loop keeps as the previous pose for gbl_render_motion_deform_device.  GBL_ERR_INVALID for a NULL
 * argument, a mesh out of range or not a triangle mesh, a range out of bounds, and the pointer refusals above. */
gbl_status gbl_get_vertices_device(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, float* d_positions_out);
/* *pending = 1 while the tie order of triangle mesh `mesh` waits for its first reader (GBL_VERTICES_DEFER_ORDER), else 0.  Host
 * only.  GBL_ERR_INVALID for a NULL argument or a mesh out of range. */
gbl_status gbl_order_pending(const gbl_ctx* ctx, uint32_t mesh, uint32_t* pending);

/* Rebuild the BLAS of triangle mesh `mesh` on the device, in place, over the positions the context holds now (gbl_create's, or
 * the last gbl_update_vertices* edit's): what a frame loop calls once a refitted tree has grown slow (gbl_mesh_tree_stats),
 * instead of re-creating the context and losing its pools, pilot, planes and history.
 *  - Afterwards every table the kernels read is what gbl_create_ex(..., GBL_CREATE_DEVICE_BVH) makes for this mesh over the same
 *    positions, whichever builder made the context: the mesh's triangles in the new Morton order (its range of the triangle
 *    table does not move), their bounds, and the linear BVH's nodes.  A render equals, bit for bit, that of a device-built
 *    context created from the deformed scene.
 *  - The tree goes into a slot of tri_count node records appended to the node array at the mesh's first rebuild (one device
 *    allocation and a device-to-device copy; every index stays valid) and reused by every later one; the builder's scratch is
 *    kept and grown on demand, so a rebuild per pose allocates nothing.  The records the old tree occupied stay unreferenced.
 *    A mesh of four triangles or fewer is one leaf and needs no slot.
 *  - Order of the call: synchronise; the slot; the build kernels (a 64-bit radix sort, and one 8-byte read-back per level of
 *    the tree); the triangle bounds; the TLAS on the host as in every edit; synchronise.  GBL_SCHEDULE_AUTO measures its rays
 *    per path again, and gbl_info.blas_depth becomes the deepest tree any mesh of the context has had.
 *  - The tie order is indexed by original triangle and is neither read nor written: a deferred order stays deferred.
 *  - The mesh's refit plan is dropped; the next gbl_update_vertices* makes it over the new tree.
 *  - Limit: in a host-built context the rebuilt tree's top nodes are no longer among the hot prefix the lean kernels keep in LDS.
 * flags is reserved and must be 0.  GBL_ERR_INVALID, the context untouched: a NULL ctx, a mesh out of range or a sphere or a
 * disk, non-zero flags.  GBL_ERR_UNSUPPORTED, the context untouched: a mesh an area light emits from (its emitting triangles
 * are listed by their place in the triangle table, and such a mesh cannot have been edited).  Scenes with a directional or image
 * based light are not refused: nothing those lights read changes. */
gbl_status gbl_rebuild_mesh(gbl_ctx* ctx, uint32_t mesh, uint32_t flags);

/* The size and the expected traversal cost of the BLAS of triangle mesh `mesh` as it is now.  The three counts come from the
 * mesh's refit plan (made here if no edit has made it: one download of the node array); the three sums are taken on the device
 * over the QUANTISED child boxes -- the boxes traversal tests: a slot's corner on axis a is o[a] + (float)q * scale[a] in float32,
 * its area dx * dy + dy * dz + dz * dx in double.  node_area / root_area is then the expected number of interior children a
 * ray that enters the root visits, tri_area / root_area the expected number of triangles it tests: both grow as a refitted tree
 * degrades, and a caller rebuilds (gbl_rebuild_mesh) when they have grown too far.  No atomics: two calls return the same bits.
 * A mesh whose root is a leaf reports nodes = levels = 0, leaves = 1 and zero sums.  Synchronises the device.
 * GBL_ERR_INVALID for a NULL argument, a mesh out of range or a sphere or a disk. */
typedef struct gbl_tree_stats {
    uint32_t nodes;      /* interior (4-wide) nodes reached from the mesh's root */
    uint32_t levels;     /* levels of them, the root's included */
    uint32_t leaves;     /* leaf slots: groups of one to four triangles */
    uint32_t reserved;
    double root_area;    /* area of the union of the root's used slots */
    double node_area;    /* sum over the used interior child slots of every node */
    double tri_area;     /* sum over the leaf slots of triangle count * area */
} gbl_tree_stats;
gbl_status gbl_mesh_tree_stats(gbl_ctx* ctx, uint32_t mesh, gbl_tree_stats* out);
/* Self-test hook: copy records [first, first + count) of a device geometry table to host memory; *total receives the table's
 * record count.  table: 0 nodes (DevNode, 64 B), 1 tris (DevTri, 48 B), 2 tri_bounds (DevTriBound, 32 B), 3 tri_order (16 B).
 * A fifth table, 4 mesh_root (int32, 4 B per mesh of the scene: the BLAS root reference an instance of the mesh carries),
 * is the context's host copy.  out may be NULL when count is 0.  Synchronises the device. */
gbl_status gbl_selftest_geometry(gbl_ctx* ctx, int table, uint64_t first, uint64_t count, void* out, uint64_t* total);

/* Camera edit: every later call on the context sees `camera`; film and resolution stay the context's.  Host work only (the
 * scene is neither rebuilt nor uploaded) and no device synchronisation: every kernel receives the camera by value, so work
 * already queued keeps the old one.  A thin lens or an orthographic camera switches the calls to the kernels that know them,
 * a pinhole back to the lean ones; the lens disk a scene file adds beside a thin lens is an instance and stays the scene's.
 * GBL_SCHEDULE_AUTO measures its rays per path again.  GBL_ERR_INVALID, the context unchanged, for a NULL argument, a type
 * beyond GBL_CAMERA_ORTHOGRAPHIC and a non-finite position, orientation or fov_degrees.  gbl_get_camera returns the
 * description last set, gbl_create's at first. */
gbl_status gbl_update_camera(gbl_ctx* ctx, const gbl_camera* camera);
gbl_status gbl_get_camera(const gbl_ctx* ctx, gbl_camera* out);

/* Light edit: lights [first, first + count) take the given records (host memory).  After GBL_OK the light records, the light
 * pick CDF and the pick probabilities on the device are byte for byte what gbl_create builds from the context's current
 * description with those lights replaced, and every render, AOV pass and query queued afterwards equals the same call on such a
 * fresh context, bit for bit.
 *  - What may change, by type.  Point: color, position.  Spot: color, position, direction, cos_theta_max, cos_falloff_start.
 *    Directional: color, direction (its power is taken over the scene bound the context was created with; every edit that could
 *    change that bound is refused in a scene with such a light).  Area: color, to_world.  Image based: to_world.orientation (the
 *    constructor's pre-rotation is applied as gbl_create applies it; the sampling distribution and the average radiance stay).
 *  - What may not: type, mesh, sample_num and image fix the Whitted quota, the stream sampler's layout, the choice of kernels
 *    and the emitting triangles, and must equal the context's values (gbl_get_lights returns them).
 *  - An edit that moves no instance packs the three tables on the host and queues their uploads on `stream` (a hipStream_t, NULL
 *    for the null stream) from pinned staging the context owns.  No kernel is launched and the device is not synchronised: work
 *    queued on that stream before the call keeps the old lights, work queued after it sees the new ones.  A caller who renders
 *    on another stream orders the two itself.  The staging has four slots; a fifth edit waits for the first one's upload.
 *  - A changed to_world on an area light also moves every instance whose area_light names it, through gbl_update_instances' own
 *    path: records, bounds, the TLAS rebuilt on the host (with gbl_update_instances' limit on the hot prefix), gbl_info.  This
 *    synchronises the device, as gbl_update_instances does, and gbl_get_instances reports the new transform afterwards, so
 *    gbl_render_motion carries the moved emitter like any other instance.  It is accepted only while each of those instances'
 *    transforms is bitwise the light's (a scene file's emissive model is loaded that way, and stays that way after an edit).
 *    gbl_update_instances on such an instance stays refused.
 *  - GBL_SCHEDULE_AUTO measures its rays per path again.
 * Refusals, in this order, nothing uploaded and the context untouched: GBL_ERR_INVALID for a NULL ctx or lights; GBL_ERR_INVALID
 * for a range past the context's lights; per light of the range GBL_ERR_INVALID for a type, mesh, sample_num or image that is
 * not the context's, naming the light and the field, and GBL_ERR_UNSUPPORTED for a different color on an image based light
 * (it is baked into the texels when the scene is loaded); per light GBL_ERR_INVALID for a float that is not finite in a field
 * the light's type may change, and for a spot or directional direction of (0, 0, 0); then for a moved area light
 * GBL_ERR_UNSUPPORTED in a scene with a directional or image based light (gbl_update_instances' refusal, with this entry's
 * name), GBL_ERR_UNSUPPORTED for a carrying instance whose transform is not the light's, and GBL_ERR_INVALID for a transform
 * the reference cannot invert (gbl_update_instances' |det| < 1e-5 refusal).  Every other value gbl_create accepts is accepted,
 * a light without power among them.  count == 0 with a valid pointer is GBL_OK and changes nothing. */
gbl_status gbl_update_lights(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_light* lights /* host */, void* stream);
/* The light records the context holds now for lights [first, first + count): gbl_create's at first, the edited ones after
 * gbl_update_lights.  Host only.  GBL_ERR_INVALID for a NULL argument or a range out of bounds. */
gbl_status gbl_get_lights(const gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_light* out /* host */);
/* Self-test hook: every DevLight record (192 B: type, color[3], pos[3], cos_max, axis[3], cos_falloff, m[12], inv[12], tri_first,
 * tri_count, sum_area, shape, radius, wh_n, wh_prefix, image, dist_offset, dist_w, dist_h, pad), the lights + 1 floats of the
 * pick CDF and the max(1, lights) pick probabilities to host memory, and *total (the light count).  Any out pointer may be NULL.
 * Synchronises the device when it copies. */
gbl_status gbl_selftest_lights(gbl_ctx* ctx, void* records_out, float* cdf_out, float* pick_pdf_out, uint64_t* total);

/* Material edit: materials [first, first + count) take the given records (host memory); the texture edit below does the same for
 * the nodes of the texture graph.  These replace what the reference can only do by loading the scene again: createLambertMaterial
 * .. createSubsurfaceMaterial (GoblinMaterial.cpp:826-927) and the texture creators (GoblinTexture.cpp:617-745) run once, when the
 * scene file is read.  After GBL_OK and in stream order the material and texture records on the device are byte for byte what
 * gbl_create packs from the context's current description with those records replaced, and every render, AOV pass and query
 * queued afterwards equals the same call on such a fresh context, bit for bit.
 *  - What may change in a material: color, color2, color3, index, k, exponent (by type as gbl_material lists them: a mask's alpha
 *    and transparent colour, a subsurface material's sigma_a, sigma_s', Kr, eta and g among them; the "Kd" + "mean_free_path" form
 *    stays the loader's), and the texture index held in an OCCUPIED slot.  What may not: type, masked_material, and whether each
 *    of the six slots (tex_color, tex_color2, tex_exponent, tex_color3, tex_bump, tex_normal) is occupied (>= 0) or not (-1):
 *    these decide DevInstance::is_mask, has_masks, has_bssrdf and the choice between the lean and the EXT kernels.
 *  - What may change in a texture: value, uv_scale, uv_offset, to_tex, max_anisotropy.  What may not: type, is_float, child,
 *    mapping, image, filter, image_filter, address.
 *  - A mask's device record carries the slot state of the material it wraps: an edit of the wrapped material packs those masks
 *    again as well.
 *  - The records are packed on the host and their uploads are queued on `stream` (a hipStream_t, NULL for the null stream) from
 *    pinned staging the context owns.  No kernel is launched and the device is not synchronised: work queued on that stream
 *    before the call keeps the old values, work queued after it sees the new ones.  A caller who renders on another stream orders
 *    the two itself.  The staging has four slots per table; a fifth edit waits for the first one's upload.  (One exception: the
 *    first host-form edit or gbl_get_* after a device-form edit downloads the rows that edit wrote, behind a synchronise.)
 *  - gbl_film_accumulate keeps its history across the edit, as across a light edit.  GBL_SCHEDULE_AUTO measures its rays per
 *    path again.
 * Refusals, in this order, nothing uploaded and the context untouched: GBL_ERR_INVALID for a NULL ctx or pointer; GBL_ERR_INVALID
 * for a range past the context's records; per record GBL_ERR_INVALID for a fixed field that is not the context's, naming the
 * record, the field and both values; per record GBL_ERR_INVALID for an editable float that is not finite (color3 counts in a
 * subsurface material only), naming the field, and for a spherical checkerboard's or image texture's to_tex that the reference
 * cannot invert (|det| < 1e-5, pack_transform's refusal); then for a slot that names another texture GBL_ERR_INVALID for a
 * texture of the other kind (tex_exponent and tex_bump take float textures, the others colour textures), and validate_desc's
 * refusals on the patched table: GBL_ERR_INVALID for an index out of range or a cyclic graph, GBL_ERR_UNSUPPORTED for a graph
 * deeper than GBL_TEX_MAX_DEPTH below the slot.  count == 0 with a valid pointer is GBL_OK and changes nothing. */
gbl_status gbl_update_materials(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_material* materials /* host */, void* stream);
gbl_status gbl_update_textures(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_texture* textures /* host */, void* stream);
/* The records the context holds now: gbl_create's at first, the edited ones after.  Host only, but for the first call after a
 * device-form edit, which downloads the rows that edit wrote once (it synchronises the device).  GBL_ERR_INVALID for a NULL
 * argument or a range out of bounds. */
gbl_status gbl_get_materials(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_material* out /* host */);
gbl_status gbl_get_textures(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_texture* out /* host */);
/* The same edits with the editable floats read from DEVICE memory: what an optimiser or an animation step on the GPU leaves
 * behind goes into the context without a trip through the host (the constructors cited above, again).  d_rows holds `count` rows,
 * 4-byte aligned: a material row is 12 floats {color[3], color2[3], color3[3], index, k, exponent}, a texture row 7 floats
 * {value[3], uv_scale[2], uv_offset[2]}; slot indices, to_tex and max_anisotropy stay with the host forms.  One kernel with one
 * lane per record reads the live record, keeps every fixed field and writes the editable ones with the packer's own arithmetic:
 * after the call and in stream order the records are byte for byte what gbl_update_materials / gbl_update_textures leave when
 * fed the same floats -- color3 stays zero outside a subsurface material, a float texture's value[0] is broadcast, a subsurface
 * material's A is worked out from index (BSSRDF ctor, GoblinMaterial.cpp:32-38) and its row's exponent is ignored.
 *  - Asynchronous on `stream`, nothing is synchronised.  The VALUES ARE NOT INSPECTED: a NaN or an infinity in a row goes into
 *    the record as it is, as gbl_update_image_device does not look at texels and gbl_create does not look at material values.
 *  - The context's host copy becomes a mirror: the edit marks its range stale, and gbl_get_materials / gbl_get_textures and the
 *    host forms refresh it with one download of the union of the stale ranges, behind a synchronise, when they need it.  The raw
 *    rows are kept in a device table made from the host copy at the first device-form edit (which allocates, and uploads it on
 *    `stream`) and written by every edit of either form after that.
 * Refusals, nothing launched and the context untouched: GBL_ERR_INVALID for a NULL ctx or pointer, a range past the context's
 * records, a pointer that is not device or managed memory of the context's device (a plain host pointer is refused before
 * anything reads it), an allocation that ends before the rows' bytes. */
gbl_status gbl_update_materials_device(gbl_ctx* ctx, uint32_t first, uint32_t count, const float* d_rows /* device, 12 * count */, void* stream);
gbl_status gbl_update_textures_device(gbl_ctx* ctx, uint32_t first, uint32_t count, const float* d_rows /* device, 7 * count */, void* stream);
/* Self-test hook: every DevMaterial record (88 B: type, color[3], color2[3], index, k, exponent, tex_color, tex_color2,
 * tex_exponent, has_tex, masked, color3[3], tex_color3, tex_bump, tex_normal, pad) and every DevTexture record (120 B: type,
 * is_float, value[3], child[2], mapping, filter, uv_scale[2], uv_offset[2], to_tex[12], image, address, max_aniso, pad[2]) to
 * host memory, and the two counts.  Any out pointer may be NULL.  Synchronises the device when it copies. */
gbl_status gbl_selftest_materials(gbl_ctx* ctx, void* materials_out, void* textures_out, uint64_t* num_materials, uint64_t* num_textures);

/* Image edit: image `image` of gbl_scene_desc.images takes a new level 0 and the MIP levels above it are built again on the
 * device.  level0 holds width * height * channels floats in level 0's layout as the context holds that image -- what the loader
 * leaves behind: texels already through ImageTexture::convertTexel (channel pick and gamma done), sides already powers of two, a
 * 4-channel image carrying its alpha, a float texture one channel.  Width, height, levels, channels and the image's place in
 * the texel pool stay.  After GBL_OK and in stream order the image's texels on the device are what gbl_create uploads for a
 * description holding this level 0 under a pyramid built as the loader builds it (level 0 the caller's, copied verbatim; level
 * l >= 1 resizeImage of level l - 1; alpha 1 on every level >= 1), bit for bit for finite level-0 texels whose pyramid stays
 * finite, and every render, AOV pass and query queued afterwards equals the same call on such a fresh context, bit for bit.
 * Non-finite texels are not validated (gbl_create does not validate them either): where the host's pyramid has a NaN the
 * device's has one too, of unspecified bits.
 *  - Both forms are asynchronous on `stream` (a hipStream_t, NULL for the null stream) and synchronise nothing: work queued on
 *    that stream before the call keeps the old image, work queued after it sees the new one.  A caller who renders on another
 *    stream orders the two itself.
 *  - gbl_update_image_device copies level 0 device to device and launches one kernel per level.  gbl_update_image differs only
 *    in copying level 0 from the caller's (pageable) host memory, which is read before the call returns.
 *  - resizeImage's tap weights depend on the level sizes only: the host computes them at the image's first edit, with the expf
 *    the loader uses, and the context keeps them on the device (that first edit allocates, and uploads them on `stream`).
 *  - GBL_SCHEDULE_AUTO measures its rays per path again: a mask's alpha may be read from an image.
 * Refusals, in this order, nothing queued and the context untouched: GBL_ERR_INVALID for a NULL ctx or pointer; GBL_ERR_INVALID
 * for an image past the context's images (every image of a scene without any); for the device form a pointer that is not device
 * or managed memory of the context's device, or whose allocation ends before level 0's bytes (GBL_ERR_INVALID; a plain host
 * pointer is refused before anything reads it); GBL_ERR_UNSUPPORTED, naming the light, for an image that a GBL_LIGHT_IBL light
 * reads -- also when a texture reads it as well: the light's sampling distribution, average radiance and power are packed from
 * these texels when the context is created; gbl_update_environment* below is the edit for such an image.  An image that nothing
 * reads is accepted. */
gbl_status gbl_update_image_device(gbl_ctx* ctx, uint32_t image, const float* d_level0 /* device */, void* stream);
gbl_status gbl_update_image(gbl_ctx* ctx, uint32_t image, const float* level0 /* host */, void* stream);
/* The image as the context holds it now: its record into *info_out and / or its whole pyramid -- level 0 first, each level
 * row-major, the sum over the levels of max(1, w >> l) * max(1, h >> l) * channels floats -- into texels_out (host memory).
 * info_out->texel_offset is 0: it counts from the start of texels_out.  Either pointer may be NULL; copying texels
 * synchronises the device.  GBL_ERR_INVALID, nothing touched, for a NULL ctx, an image out of range, and two NULL pointers. */
gbl_status gbl_get_image(gbl_ctx* ctx, uint32_t image, gbl_image* info_out /* or NULL */, float* texels_out /* host, or NULL */);

/* Environment edit: the image of image based light `light` takes a new level 0, and everything gbl_create derives from those
 * texels is made again on the device.  The edit is addressed by light: it changes the light's tables, not only texels.  level0
 * holds width * height * 4 floats in the layout in which the context holds the light's image -- what the loader leaves behind:
 * sides already powers of two, the light's `filter` colour already multiplied in.  Nothing validates the texels, as in
 * gbl_create.  After GBL_OK and in stream order these tables equal what a fresh gbl_create holds for a description that differs
 * only in this level 0 under a pyramid built as the loader builds it -- bit for bit wherever the host's value is not a NaN, and a
 * NaN of unspecified bits where it is one (a row or an image that sums to zero makes the host's own CDF 0 / 0):
 *   1. the image's whole pyramid in the texel pool, as gbl_update_image* builds it;
 *   2. the light's sampling distribution (luminance * sin(theta) of pyramid level max(0, levels - 9), neither side above 256): the
 *      marginal block over the rows' integrals, then one block per row, each func[n], cdf[n + 1], integral;
 *   3. the light's power (the 1 x 1 level's radiance over the sphere of the scene bound the context was created with), and with it
 *      the light pick CDF and the pick probabilities of every light.
 * The light's record does not change: where its distribution lies and its size depend on the image's size only.  A texture that
 * reads the same image sees the new texels.
 *  - Both forms queue everything on `stream` (a hipStream_t, NULL for the null stream) and synchronise nothing: work queued on
 *    that stream before the call keeps the old environment, work queued after it sees the new one.  gbl_update_environment differs
 *    only in copying level 0 from the caller's (pageable) host memory, which is read before the call returns.
 *  - The light's first edit makes sin(theta) per row of its distribution on the host, with the sinf gbl_create uses, and uploads
 *    it on `stream`; the image's first edit does the same for the pyramid's tap weights; the context's first edit puts the lights'
 *    powers on the device.  These first edits allocate.
 *  - The host does not know the light's new power: it is worked out on the device and copied into pinned memory behind an event.
 *    gbl_update_lights, which packs the pick distribution on the host, waits for that event before it packs -- the one host wait
 *    this entry adds, paid by the next gbl_update_lights and not by the edit, and over once the edit's kernels have run.
 *    gbl_update_lights after an environment edit, and the two in the other order, leave the tables of a fresh context given both.
 *  - GBL_SCHEDULE_AUTO measures its rays per path again.
 * Refusals, in this order, nothing queued and the context untouched: GBL_ERR_INVALID for a NULL ctx or pointer; GBL_ERR_INVALID
 * for a light past the context's lights; GBL_ERR_INVALID, naming its type, for a light that is not a GBL_LIGHT_IBL; for the
 * device form a pointer that is not device or managed memory of the context's device, or whose allocation ends before level 0's
 * bytes (GBL_ERR_INVALID; a plain host pointer is refused before anything reads it); GBL_ERR_UNSUPPORTED, naming it, when another
 * image based light reads the same image.  Two image based lights over two images are edited one after the other. */
gbl_status gbl_update_environment_device(gbl_ctx* ctx, uint32_t light, const float* d_level0 /* device */, void* stream);
gbl_status gbl_update_environment(gbl_ctx* ctx, uint32_t light, const float* level0 /* host */, void* stream);
/* Self-test hook: the light's block of the distribution table to host memory -- (2 h + 2) + h (2 w + 2) floats for a distribution
 * of w x h, the count also in *dist_floats -- and {pyramid level, w, h} in dims_out.  Any out pointer may be NULL; copying
 * synchronises the device.  GBL_ERR_INVALID for a NULL ctx, a light out of range and a light that is not image based. */
gbl_status gbl_selftest_environment(gbl_ctx* ctx, uint32_t light, float* dist_out /* host, or NULL */, uint64_t* dist_floats,
                                    uint32_t dims_out[3] /* level, dist_w, dist_h; or NULL */);

/* Scene queries: Scene::intersect (GBL_QUERY_CLOSEST) or Scene::occluded (GBL_QUERY_ANY) for n caller rays in DEVICE memory,
 * against the context as it is now -- every gbl_update_instances*, gbl_update_vertices*, gbl_rebuild_mesh edit taken so far is
 * seen.  What a simulation step on the GPU asks between two edits: collision probes, ground snapping, line of sight, picking,
 * probe and lightmap baking, custom AO.
 *  - A ray is {o, mint, d, maxt}.  d need not be normalised and t is in units of d: o = p, d = q - p, mint = eps, maxt = 1 - eps
 *    asks "does q see p".  maxt = +inf is allowed.  The interval is inclusive, like the reference's.
 *  - GBL_QUERY_CLOSEST writes n gbl_ray_hit records.  On a hit: t, b1, b2 as the triangle test left them; instance indexes
 *    gbl_scene_desc.instances; primitive is the triangle's number within its own mesh in the scene description's order (it does
 *    not change when a builder or gbl_rebuild_mesh reorders the triangle table); a sphere or a disk reports primitive 0 and
 *    b1 = b2 = 0.  On a miss: t = -1, instance = -1, everything else 0.  The hit point is o + t d, or the mesh's
 *    v0 + b1 (v1 - v0) + b2 (v2 - v0) taken to world space.
 *  - GBL_QUERY_ANY writes n bytes: 1 occluded, 0 not.
 *  - GBL_QUERY_SHADING_NORMAL (closest only): n is the world-space shading normal of the hit -- interpolated vertex normals
 *    where the mesh has them, bump and normal maps applied, unit length, NOT flipped towards the ray.  Without the flag n is
 *    zeros and no fragment is made.
 *  - GBL_QUERY_EXACT_TIES: the reference's answer bit for bit, as a render with exact_ties: its visiting order decides which of
 *    two triangles met at exactly the same t is reported, and a triangle its own (not watertight) box tests would pass by is
 *    not accepted.  Without the flag the nearest accepted triangle is reported, whichever of two tied ones was tested last;
 *    never a hit farther than the exact one's, and never a miss where the exact query hits.  Which builds read the tie order
 *    (gbl_update_vertices_device): the two exact ones only.  A query without the flag -- on a scene of the headline feature set
 *    or on one with analytic shapes -- does not, and leaves a deferred order pending.
 *  - An invalid ray -- a NaN among its eight floats, an infinite component of o or d, d all zeros, !(mint <= maxt) -- reports a
 *    miss (unoccluded) and enters no traversal.  No input makes the call spin: traversal is bounded by its stack.
 *  - Asynchronous on `stream`; no host synchronisation but these: the one that makes a pending tie order for an exact query; in a
 *    context's first query, one small upload and the allocation of the stack backing; and, in the first query after an edit has
 *    deepened the tree past that backing, its reallocation (a free and an allocation, which wait for the device).  The per-lane
 *    stacks beyond 16 levels live in that buffer of the context: queries of one context are queued on one stream at a time, like
 *    its renders.
 *  - Queries of this entry are unfiltered: the surface of a mask material counts as a surface.  The reference's isOpaque /
 *    notOpaque filters and the transmittance its shadow rays take are gbl_trace_rays_filtered's, below.
 * Refusals, nothing launched: GBL_ERR_INVALID for a NULL ctx, a NULL pointer with n > 0, an unknown kind, unknown bits in flags,
 * GBL_QUERY_SHADING_NORMAL with GBL_QUERY_ANY, a pointer that is not device or managed memory of the context's device (a plain
 * host pointer is refused before anything reads it) or whose allocation ends before 32 n bytes (n bytes for the any-hit
 * output), and d_out overlapping d_rays; GBL_ERR_UNSUPPORTED for n >= 2^32 (the kernel keeps 32-bit ray indices).  n == 0 is
 * GBL_OK and does nothing, whatever the pointers. */
typedef struct gbl_ray     { float o[3]; float mint; float d[3]; float maxt; } gbl_ray;      /* 32 B: two 16-byte loads */
typedef struct gbl_ray_hit { float t, b1, b2; int32_t instance; uint32_t primitive; float n[3]; } gbl_ray_hit; /* 32 B */
#define GBL_QUERY_CLOSEST 0u      /* Scene::intersect */
#define GBL_QUERY_ANY     1u      /* Scene::occluded  */
#define GBL_QUERY_EXACT_TIES      1u   /* flags */
#define GBL_QUERY_SHADING_NORMAL  2u
gbl_status gbl_trace_rays(gbl_ctx* ctx, uint32_t kind, const gbl_ray* d_rays, uint64_t n,
                          void* d_out /* CLOSEST: n gbl_ray_hit; ANY: n bytes, 1 = occluded */,
                          uint32_t flags, void* stream);
/* Self-test hook: gbl_trace_rays on the default stream with its persistent grid capped at max_workgroups (0: no cap) and a
 * device synchronise at the end.  With one workgroup each wave walks many 64-ray regions at a few thousand rays: the refill
 * path a plain call only reaches at hundreds of thousands of rays. */
gbl_status gbl_selftest_query(gbl_ctx* ctx, uint32_t kind, const gbl_ray* d_rays, uint64_t n, void* d_out, uint32_t flags,
                              uint32_t max_workgroups);

/* Filtered scene queries: gbl_trace_rays under the reference's IntersectFilter, and the transmittance of a shadow segment as
 * PathTracer::Li takes it -- what a caller's shadow rays need to agree with the integrator in a scene of cut-outs, tinted panes and
 * decals.  Rays, records, flags, stream order, synchronisation points and refusals are gbl_trace_rays'; what is added:
 *  - filter, for GBL_QUERY_CLOSEST and GBL_QUERY_ANY.  GBL_QUERY_FILTER_NONE is gbl_trace_rays itself: the same kernels, the same
 *    bytes.  GBL_QUERY_FILTER_OPAQUE skips every instance whose material is a mask (or a subsurface material, which the
 *    reference marks the same way) whole, as Model::intersect does under isOpaque; GBL_QUERY_FILTER_MASK skips every other
 *    instance (notOpaque).  The answer is that of gbl_trace_rays on a scene with the skipped instances removed, `instance` still
 *    numbering the whole scene's.  An instance is on one side by its material's TYPE: a mask whose alpha is 1 is still a mask.
 *  - kind GBL_QUERY_TRANSMITTANCE (filter must be GBL_QUERY_FILTER_NONE, GBL_QUERY_SHADING_NORMAL is refused) writes n
 *    gbl_ray_transmittance records.  If an opaque surface lies within [mint, maxt] -- Scene::occluded(ray, isOpaque) -- tr is
 *    {0, 0, 0} and crossed is 0x80000000.  Otherwise tr is PathTracer::evalAttenuation's product over the mask surfaces of the
 *    segment, front to back: (1 - alpha) * transparent_color per surface, alpha and colour looked up at the hit as a render does,
 *    mint moved to t + epsilon behind each; the walk ends at Black (a mask that wraps a subsurface material answers Black) or
 *    after 1024 surfaces; crossed counts the factors multiplied in.  An invalid ray answers {1, 1, 1}, 0.
 *    GBL_QUERY_EXACT_TIES governs the occlusion query; the walk's own closest-hit queries follow the reference's tie rule always,
 *    as a render's do, so a pending tie order is made (one synchronisation) by every transmittance query.
 *  - A scene without a mask material launches no filtered traversal: OPAQUE is NONE, MASK misses everywhere, TRANSMITTANCE is the
 *    any-hit answer rewritten as {1, 1, 1}, 0 or {0, 0, 0}, 0x80000000 (through n bytes of the context's own, grown on demand).
 *  - Limit: where two instances on the same side of the filter are met at exactly the same t, which one is reported is the
 *    traversal order's choice, as in gbl_trace_rays; DESIGN.md 4.11.
 * Further refusals, nothing launched: GBL_ERR_INVALID for an unknown filter, for GBL_QUERY_TRANSMITTANCE with a filter other than
 * GBL_QUERY_FILTER_NONE or with GBL_QUERY_SHADING_NORMAL, and for a transmittance output whose allocation ends before 16 n bytes. */
#define GBL_QUERY_FILTER_NONE   0u
#define GBL_QUERY_FILTER_OPAQUE 1u   /* instances whose material is a mask are skipped whole: Model::intersect under isOpaque */
#define GBL_QUERY_FILTER_MASK   2u   /* only those instances: notOpaque */
#define GBL_QUERY_TRANSMITTANCE 2u   /* kind, accepted by gbl_trace_rays_filtered only */
typedef struct gbl_ray_transmittance { float tr[3]; uint32_t crossed; } gbl_ray_transmittance;  /* 16 B */
gbl_status gbl_trace_rays_filtered(gbl_ctx* ctx, uint32_t kind, uint32_t filter, const gbl_ray* d_rays, uint64_t n,
                                   void* d_out /* CLOSEST: n gbl_ray_hit; ANY: n bytes; TRANSMITTANCE: n gbl_ray_transmittance */,
                                   uint32_t flags, void* stream);
/* Self-test hook: gbl_trace_rays_filtered as gbl_selftest_query is gbl_trace_rays. */
gbl_status gbl_selftest_query_filtered(gbl_ctx* ctx, uint32_t kind, uint32_t filter, const gbl_ray* d_rays, uint64_t n, void* d_out,
                                       uint32_t flags, uint32_t max_workgroups);

/* Path-traced radiance along caller rays: PathTracer::Li (GoblinPathtracer.cpp:50-179) for n rays in device memory, against the
 * scene as every edit so far left it -- what a probe, a lightmap texel, a rasteriser's reflection pass or a second view asks, without
 * re-aiming the scene's one camera and reading a film back.
 *  - Ray i is the ray Li receives: its first query is Scene::intersect over [mint, maxt] (maxt = +inf is the usual value), and a
 *    first query that ends without a surface adds the environment as :61-65 does.  d must be a unit vector (every BSDF reads
 *    wo = -d).  No vertex has ray differentials: the ray is a RayDifferential without auxiliary rays (GoblinRay.h:48-51), which
 *    is what every continuation ray of the reference is, so trilinear and EWA lookups at vertex 0 see a zero footprint.  If the rays
 *    are a frame's own camera rays, the answers are that frame's per-sample Li (gbl_render's li_out) bit for bit, but for those
 *    lookups.
 *  - d_out[i] = {Li.r, Li.g, Li.b, 1}.  A NaN component is stored as it is: the caller drops it, as ImageTile::addSample does.  An
 *    invalid ray -- gbl_trace_rays' rule, or |d.d - 1| > 1e-4 -- answers {0, 0, 0, 0} and fetches no node.  A scene without lights
 *    answers {0, 0, 0, 1} for every valid ray (:53-56).
 *  - max_ray_depth is PathTracer's: the loop runs max_ray_depth - 1 times; 1 = emission / environment only.
 *  - Native draws (d_records == NULL): ray i is sample k = i % S of group g = first_group + i / S, S = samples_per_group, and
 *    draws what camera sample k of a pixel whose index in the full sample window is g draws under gbl_render_params.seed == seed
 *    at S samples per pixel: vertex b takes the 1D patterns 3 b, 3 b + 1, 3 b + 2 and the 2D patterns 0x10000 + 2 b and + 1.  So a
 *    group is to this call what a pixel is to gbl_render -- its S samples are stratified against each other -- and a batch split
 *    over calls with matching first_group draws what one call would.  GBL_RADIANCE_RUSSIAN_ROULETTE and GBL_RADIANCE_EXACT_TIES
 *    are gbl_render_params' russian_roulette and exact_ties.
 *  - Replay draws (d_records != NULL): record i is ray i's, in gbl_render's replay layout for the path tracer at this max_ray_depth
 *    in this scene (gbl_host_sample_dimension_scene floats; record_stride must equal that).  Its first four floats (image position,
 *    lens) are not read.  first_group, seed and samples_per_group are then ignored, except that n % S == 0 still holds.
 *  - Which builds read the tie order (gbl_update_vertices_device): every one but the lean native build without
 *    GBL_RADIANCE_EXACT_TIES, which leaves a deferred order pending.
 *  - Asynchronous on params->stream; no host synchronisation but gbl_trace_rays' (a pending tie order, the stack backing).  The
 *    per-lane stacks beyond 16 levels live in the query kernels' buffer of the context, so no tree is too deep for the call, and
 *    radiance calls and queries of one context are queued on one stream at a time.
 * Refusals, nothing launched: GBL_ERR_INVALID for a NULL ctx or params, reserved != 0, unknown bits in flags, max_ray_depth
 * outside [1, 16384] (above it the 1D pattern numbers reach the 2D patterns' base), samples_per_group not a perfect square in [1, 2^31),
 * n % samples_per_group != 0, first_group + n / samples_per_group past 2^32, GBL_RADIANCE_RUSSIAN_ROULETTE with records, a wrong
 * record_stride, and gbl_trace_rays' buffer refusals (the records included; d_out holds 16 n bytes); GBL_ERR_UNSUPPORTED for
 * n >= 2^32 and for a scene with a participating medium or a subsurface material: the medium and Lsubsurface are computed per
 * camera sample by kernels of their own, and radiance through fog without the fog would be silently wrong.  n == 0 is GBL_OK and
 * does nothing.  Not offered: the Whitted and AO integrators, a per-ray depth or seed, the mean of a group's samples. */
#define GBL_RADIANCE_EXACT_TIES       1u   /* lean scenes: the reference's tie rule, as gbl_render_params.exact_ties */
#define GBL_RADIANCE_RUSSIAN_ROULETTE 2u   /* the build-side extension of gbl_render_params.russian_roulette; native draws only */
typedef struct gbl_radiance_params {
    int32_t  max_ray_depth;       /* PathTracer's: the loop runs max_ray_depth - 1 times; 1 = emission / environment only */
    uint32_t samples_per_group;   /* S, a perfect square >= 1 */
    uint32_t first_group;         /* the group number of ray 0 (a batch split over calls draws what one call would) */
    uint32_t flags;
    uint64_t seed;                /* native draws */
    const float* d_records;       /* device, or NULL = native draws */
    uint32_t record_stride;       /* floats per record when d_records != NULL */
    uint32_t reserved;            /* 0 */
    void* stream;                 /* hipStream_t, NULL = default */
} gbl_radiance_params;
gbl_status gbl_radiance_rays(gbl_ctx* ctx, const gbl_ray* d_rays, uint64_t n, const gbl_radiance_params* params,
                             float* d_out /* device, n float4 */);
/* Self-test hook: gbl_radiance_rays with its persistent grid capped at max_workgroups (0: no cap) and a device synchronise at the
 * end, as gbl_selftest_query is gbl_trace_rays. */
gbl_status gbl_selftest_radiance(gbl_ctx* ctx, const gbl_ray* d_rays, uint64_t n, const gbl_radiance_params* params, float* d_out,
                                 uint32_t max_workgroups);

/* Self-test hook: the device's sinf / cosf (glibc's algorithm restated, kernels/refmath.h) on n device floats. */
gbl_status gbl_selftest_sincos(gbl_ctx* ctx, const float* in, float* sin_out, float* cos_out, uint64_t n);
/* Self-test hook: out[i] = fn(a[i] [, b[i]]) on n device floats, fn one of the libm functions the reference's sampling code
 * passes through (exp / log / log2 / pow / atan / atan2 / tan / acos on floats: glibc's algorithms restated, kernels/refmath.h).
 * b may be NULL for the one-argument functions. */
typedef enum gbl_libm_fn {
    GBL_LIBM_EXPF = 0, GBL_LIBM_LOGF = 1, GBL_LIBM_LOG2F = 2, GBL_LIBM_POWF = 3,
    GBL_LIBM_ATANF = 4, GBL_LIBM_ATAN2F = 5, GBL_LIBM_TANF = 6, GBL_LIBM_ACOSF = 7
} gbl_libm_fn;
gbl_status gbl_selftest_libm(gbl_ctx* ctx, int fn, const float* a, const float* b, float* out, uint64_t n);
/* Self-test hook: out[4 i ..] = {sqrtf(a), a / b, 1 / a, normalize(a, b, 0.5).x} on n device floats -- the basic
 * operations must round like the host's for per-sample radiance to be bit-identical with the reference. */
gbl_status gbl_selftest_arith(gbl_ctx* ctx, const float* a, const float* b, float* out, uint64_t n);
/* Self-test hook: scene queries for n device rays {kind (0 Scene::intersect, 1 Scene::occluded), o(3), d(3), mint, maxt}
 * -> out n x 8 floats {hit t or -1 | 1 occluded or 0, hit instance or -1, shading normal(3), tangent(3)}. */
gbl_status gbl_selftest_trace(gbl_ctx* ctx, const float* rays, float* out, uint32_t n);

/* Self-test hook: VALU issue-rate microbenchmark, no memory traffic.  Every CU runs one workgroup of 4 * waves_per_simd
 * waves (waves_per_simd 1..4 resident on each SIMD), every wave `iters` x 64 instructions of kind `op` over 16 independent
 * register chains.  The launch that is read follows two seconds of the same launch back to back (the chip settles its clock
 * under a load over seconds).  out[8] = {launch ms (HIP events), wave-instructions of the launch, s_memtime ticks per wave,
 * ticks per instruction of a wave, s_memrealtime (100 MHz) ticks per wave over the same span, shader clock in GHz = the ratio
 * of the two x 0.1, the longest and the shortest span of a wave in 100 MHz ticks}.  The waves of a SIMD start together but the
 * older one is served first, so they finish one after the other: a SIMD's issue rate follows from the LONGEST span (or the
 * launch time), not from the average one.  The peak the traversal kernels' issue rate is read against comes from this measurement. */
typedef enum gbl_valu_op {
    GBL_VALU_FMA_F32 = 0, GBL_VALU_PK_FMA_F32 = 1, GBL_VALU_ADD_F32 = 2, GBL_VALU_MAX3_F32 = 3, GBL_VALU_CVT_UBYTE = 4,
    GBL_VALU_PERM_B32 = 5, GBL_VALU_MOV_DPP = 6, GBL_VALU_CNDMASK = 7, GBL_VALU_AND_B32 = 8, GBL_VALU_RCP_F32 = 9,
    GBL_VALU_MED3_F32 = 10, GBL_VALU_CMP_F32 = 11, GBL_VALU_MUL_F32 = 12, GBL_VALU_FMAC_F32 = 13, GBL_VALU_MAX_F32 = 14, GBL_VALU_MOV_B32 = 15,
    GBL_VALU_ADD_U32 = 16, GBL_VALU_LSHL_B32 = 17, GBL_VALU_ADD_F32_E64 = 18, GBL_VALU_FMA_F32_2SRC = 19, GBL_VALU_MUL_LO_U32 = 20,
    GBL_VALU_MUL_U32_U24 = 21, GBL_VALU_MUL_HI_U32 = 22, GBL_VALU_XOR_B32 = 23, GBL_VALU_LSHR_B32 = 24, GBL_VALU_CNDMASK_SGPR = 25, GBL_VALU_OP_COUNT = 26
} gbl_valu_op;
gbl_status gbl_selftest_valu_issue(gbl_ctx* ctx, int op, int waves_per_simd, uint32_t iters, double* out);

void gbl_destroy(gbl_ctx* ctx);
/* Message for the last failing call on ctx (or on creation when ctx == NULL). */
const char* gbl_last_error(const gbl_ctx* ctx);
int gbl_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GOBLIN_HIP_H */
