/*
 * rtgpu.h -- C ABI of the MI355X path-tracing core (PathTracerMIS over the two-level BVH).
 *
 * This is the drop-in boundary.  The reference (Witek902/Raytracer) has no FFI: the integrator sits
 * behind the C++ virtual IRenderer::RenderPixel (Core/Rendering/Renderer.h:56) and is called once per
 * pixel from Viewport::RenderTile (Core/Rendering/Viewport.cpp:338).  A per-pixel virtual is not a GPU
 * boundary, so the seam is ONE PASS: everything Viewport::Render does between Viewport.cpp:200 and
 * Viewport.cpp:262 (per-pass sampler seeds -> tile fan-out -> RenderTile -> RenderPixel -> Film).
 *
 * Everything crossing this ABI is a plain pointer, size or POD struct.  No C++ types, no torch types,
 * no exceptions.  All functions return RTGPU_OK (0) or a negative RtgpuStatus; rtgpu_last_error()
 * returns a human readable message for the last failure on the calling thread.
 *
 * Matrices are 4 rows of 4 floats, row-vector convention exactly as rt::math::Matrix4
 * (Core/Math/Matrix4.h:20-27): point' = p.x*row0 + p.y*row1 + p.z*row2 + row3.
 */
#ifndef RTGPU_H
#define RTGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTGPU_ABI_VERSION 3u

typedef enum RtgpuStatus
{
    RTGPU_OK = 0,
    RTGPU_ERR_INVALID_ARGUMENT = -1,
    RTGPU_ERR_NO_DEVICE = -2,
    RTGPU_ERR_OUT_OF_MEMORY = -3,
    RTGPU_ERR_DEVICE = -4,      /* a HIP call failed; see rtgpu_last_error() */
    RTGPU_ERR_NOT_READY = -5,   /* e.g. render_pass before upload_scene / resize */
    RTGPU_ERR_UNSUPPORTED = -6  /* feature outside the hot-path scope (textures, decals, CSG ...) */
} RtgpuStatus;

/* sentinel ids, Core/Traversal/HitPoint.h:8-9 */
#define RT_INVALID_OBJECT 0xFFFFFFFFu
#define RT_LIGHT_OBJECT   0xFFFFFFFEu
#define RT_NO_MATERIAL    0xFFFFFFFFu

/* ---------------------------------------------------------------------------------------------
 * Scene description (flat, read-only after upload).  Replaces the pointer graph the reference walks:
 * Scene::mTraceableObjects / mLights / mGlobalLights (Core/Scene/Scene.h:83-96), BVH::mNodes
 * (Core/BVH/BVH.h:22-30), VertexBuffer (Core/Shapes/Mesh/VertexBuffer.h:18-31), Material
 * (Core/Material/Material.h:47-73).
 * ------------------------------------------------------------------------------------------- */

/* 32-byte BVH node, bit-identical to rt::BVH::Node (Core/BVH/BVH.h:22-30).
 * leaves = numLeaves (low 30 bits) | splitAxis << 30.  numLeaves != 0 <=> leaf.
 * Interior: children are nodes[childIndex], nodes[childIndex+1].
 * Leaf: items [childIndex, childIndex + numLeaves) of the owning container
 * (scene objects for the top level, triangles for a mesh). */
typedef struct RtNode
{
    float    min[3];
    uint32_t childIndex;
    float    max[3];
    uint32_t leaves;
} RtNode;

/* 36 bytes, rt::math::ProcessedTriangle (Core/Math/Triangle.h:25-41) */
typedef struct RtTriangle
{
    float v0[3];
    float edge1[3];
    float edge2[3];
} RtTriangle;

/* 16 bytes, rt::VertexIndices (Core/Shapes/Mesh/VertexBuffer.h:18-24).
 * i0..i2 are relative to the owning mesh's first vertex; materialIndex is a GLOBAL index into
 * RtSceneDesc::materials or RT_NO_MATERIAL (=> the object's default material,
 * Core/Shapes/MeshShape.cpp:288-291). */
typedef struct RtVertexIndices
{
    uint32_t i0, i1, i2;
    uint32_t materialIndex;
} RtVertexIndices;

/* 32 bytes, rt::VertexShadingData (Core/Shapes/Mesh/VertexBuffer.h:26-31) */
typedef struct RtVertexShading
{
    float normal[3];
    float tangent[3];
    float texCoord[2];
} RtVertexShading;

typedef struct RtMesh
{
    uint32_t firstNode;     /* into RtSceneDesc::meshNodes; node childIndex values are mesh-relative */
    uint32_t numNodes;
    uint32_t firstTriangle; /* into triangles[] and vertexIndices[] (same order: BVH leaf order) */
    uint32_t numTriangles;
    uint32_t firstVertex;   /* into vertexShading[] */
    uint32_t numVertices;
    uint32_t _pad[2];
} RtMesh;

typedef enum RtShapeKind
{
    RT_SHAPE_SPHERE = 0, /* param = { radius, 1/radius, 0, 0 }            Core/Shapes/SphereShape.cpp:13 */
    RT_SHAPE_BOX    = 1, /* param = { size.xyz (half extents), 0 }        Core/Shapes/BoxShape.cpp:91   */
    RT_SHAPE_RECT   = 2, /* param = { size.x, size.y, texScale.x, .y }    Core/Shapes/RectShape.cpp:14  */
    RT_SHAPE_MESH   = 3  /* meshIndex valid                               Core/Shapes/MeshShape.cpp:34  */
} RtShapeKind;

typedef enum RtObjectKind
{
    RT_OBJECT_SHAPE = 0, /* rt::ShapeSceneObject  Core/Scene/Object/SceneObject_Shape.cpp */
    RT_OBJECT_LIGHT = 1  /* rt::LightSceneObject  Core/Scene/Object/SceneObject_Light.cpp (finite lights only) */
} RtObjectKind;

/* One traceable scene object, in top-level-BVH leaf order (Core/Scene/Scene.cpp:87-95). */
typedef struct RtObject
{
    float    transform[16];     /* local -> world, ISceneObject::mTransform         */
    float    invTransform[16];  /* world -> local, Matrix4::Inverse() of the above  (SceneObject.cpp:22).  Pass the reference's OWN inverse (GetInverseTransform()):
                                   the library never recomputes it, and a differently rounded inverse changes rendered bits (1-2 ulp under general rotations) */
    uint32_t objectKind;        /* RtObjectKind */
    uint32_t shapeKind;         /* RtShapeKind (for lights: shape of the area light; unused for point/spot) */
    uint32_t materialIndex;     /* default material (shapes); RT_NO_MATERIAL for lights */
    uint32_t meshIndex;         /* RT_SHAPE_MESH only */
    uint32_t lightIndex;        /* RT_OBJECT_LIGHT only: index into RtSceneDesc::lights */
    uint32_t _pad[3];
    float    shapeParam[4];
    float    shapeParam2[4];    /* box: 1/size (w=0); others unused */
} RtObject;

typedef enum RtLightType /* rt::ILight::Type, Core/Scene/Light/Light.h:27-34 */
{
    RT_LIGHT_AREA = 0,
    RT_LIGHT_BACKGROUND = 1,
    RT_LIGHT_DIRECTIONAL = 2,
    RT_LIGHT_POINT = 3,
    RT_LIGHT_SPOT = 4
} RtLightType;

#define RT_LIGHT_FLAG_FINITE 1u /* ILight::Flag_IsFinite */
#define RT_LIGHT_FLAG_DELTA  2u /* ILight::Flag_IsDelta  */

/* One light, in Scene::mLights order (= AddObject order, Core/Scene/Scene.cpp:45-48). */
typedef struct RtLight
{
    float    transform[16];
    float    invTransform[16];
    float    color[4];       /* Spectrum::rgbValues; all FOUR lanes are significant (RayColor::AlmostZero) */
    uint32_t type;           /* RtLightType */
    uint32_t flags;          /* RT_LIGHT_FLAG_* as returned by ILight::GetFlags() */
    uint32_t shapeKind;      /* area lights: RT_SHAPE_SPHERE / BOX / RECT */
    uint32_t isDelta;        /* directional / spot: mIsDelta (cos > 0.9999, Light.h:25) */
    float    cosAngle;       /* directional / spot: cosf(angle) computed by the host */
    uint32_t texture;        /* background light: BackgroundLight::mTexture (environment map, BackgroundLight.cpp:45-61)
                              * as an index into RtSceneDesc::textures, or RT_NO_TEXTURE */
    float    _pad[2];
    float    shapeParam[4];
    float    shapeParam2[4];
} RtLight;

typedef enum RtBsdf /* string names of Material::SetBsdf, Core/Material/Material.cpp:40-83 */
{
    RT_BSDF_NULL = 0,
    RT_BSDF_DIFFUSE = 1,
    RT_BSDF_ROUGH_DIFFUSE = 2,
    RT_BSDF_DIELECTRIC = 3,
    RT_BSDF_ROUGH_DIELECTRIC = 4,
    RT_BSDF_METAL = 5,
    RT_BSDF_ROUGH_METAL = 6,
    RT_BSDF_PLASTIC = 7,
    RT_BSDF_ROUGH_PLASTIC = 8
} RtBsdf;

#define RT_NO_TEXTURE 0xFFFFFFFFu

/* ITexture implementations that can sit on the shading path (Core/Textures/). */
typedef enum RtTextureKind
{
    RT_TEXTURE_BITMAP = 0,        /* BitmapTexture  (BitmapTexture.cpp:32-93) */
    RT_TEXTURE_CHECKERBOARD = 1,  /* CheckerboardTexture (CheckerboardTexture.cpp:31-40): colorA / colorB */
    RT_TEXTURE_CONST = 2,         /* ConstTexture: colorA */
    RT_TEXTURE_NOISE = 3,         /* NoiseTexture (NoiseTexture.cpp:58-164): simplex noise octaves, Lerp(colorA, colorB, value) */
    RT_TEXTURE_MIX = 4            /* MixTexture (MixTexture.cpp:23-30): Lerp(textures[mixA], textures[mixB], textures[mixWeight]);
                                   * a mix may reference mixes one level deep (rtgpu_upload_scene rejects deeper nesting) */
} RtTextureKind;

/* Texel formats: the values of rt::Bitmap::Format (Core/Utils/Bitmap.h:15-41), every one decoded on the device exactly
 * as Bitmap::GetPixel / GetPixelBlock do (Bitmap.cpp:335-832, Math/Packed.h, Utils/BlockCompression.cpp).  The
 * block-compressed formats address whole 4 x 4 blocks (width / 4 blocks per row, like the reference). */
typedef enum RtBitmapFormat
{
    RT_FORMAT_R8_UNORM = 1, RT_FORMAT_R8G8_UNORM = 2, RT_FORMAT_B8G8R8_UNORM = 3, RT_FORMAT_B8G8R8A8_UNORM = 4,
    RT_FORMAT_R8G8B8A8_UNORM = 5, RT_FORMAT_B8G8R8A8_UNORM_PALETTE = 6, RT_FORMAT_B5G6R5_UNORM = 7,
    RT_FORMAT_R16_UNORM = 8, RT_FORMAT_R16G16_UNORM = 9, RT_FORMAT_R16G16B16A16_UNORM = 10,
    RT_FORMAT_R32_FLOAT = 11, RT_FORMAT_R32G32_FLOAT = 12, RT_FORMAT_R32G32B32_FLOAT = 13, RT_FORMAT_R32G32B32A32_FLOAT = 14,
    RT_FORMAT_R11G11B10_FLOAT = 15,
    RT_FORMAT_R16_HALF = 16, RT_FORMAT_R16G16_HALF = 17, RT_FORMAT_R16G16B16_HALF = 18, RT_FORMAT_R16G16B16A16_HALF = 19,
    RT_FORMAT_R9G9B9E5_SHAREDEXP = 20, RT_FORMAT_BC1 = 21, RT_FORMAT_BC4 = 22, RT_FORMAT_BC5 = 23
} RtBitmapFormat;

typedef enum RtTextureFilter /* BitmapTextureFilter, Core/Textures/BitmapTexture.h */
{
    RT_FILTER_NEAREST = 0, RT_FILTER_BILINEAR = 1, RT_FILTER_BILINEAR_SMOOTHSTEP = 2
} RtTextureFilter;

/* 96 bytes */
typedef struct RtTexture
{
    uint32_t kind;          /* RtTextureKind */
    uint32_t format;        /* RtBitmapFormat */
    uint32_t width, height;
    uint32_t stride;        /* bytes per row, Bitmap::mStride (unused by the block-compressed formats) */
    uint32_t linearSpace;   /* Bitmap::mLinearSpace; 0 => Convert_sRGB_To_Linear on every fetched texel (all four lanes) */
    uint32_t filter;        /* RtTextureFilter */
    uint32_t numOctaves;    /* noise */
    uint64_t dataOffset;    /* byte offset of the first row (or block) in RtSceneDesc::texelData */
    uint64_t paletteOffset; /* palette format: byte offset of the B8G8R8A8 palette entries in texelData */
    float    colorA[4];     /* checkerboard / const / noise */
    float    colorB[4];
    uint32_t mixA, mixB, mixWeight;   /* mix: indices into RtSceneDesc::textures */
    uint32_t _pad;
} RtTexture;

/* 80 bytes; rt::Material after Compile() (Core/Material/Material.cpp:105-117): scalar parameters, the textures of the
 * four MaterialParameters (value = baseValue * texture->Evaluate(uv), MaterialParameter.h:22-32) and the normal map
 * (Material::GetNormalVector, Material.cpp:120-138; applied in Scene::EvaluateIntersection, Scene.cpp:327-337). */
typedef struct RtMaterial
{
    float    emission[4];   /* all four lanes significant */
    float    baseColor[4];
    float    roughness;
    float    metalness;
    float    IoR;
    float    K;
    uint32_t bsdf;          /* RtBsdf */
    uint32_t baseColorTexture;   /* indices into RtSceneDesc::textures, or RT_NO_TEXTURE */
    uint32_t emissionTexture;
    uint32_t roughnessTexture;
    uint32_t metalnessTexture;
    uint32_t normalMapTexture;
    float    normalMapStrength;
    uint32_t _pad;
} RtMaterial;

typedef struct RtSceneDesc
{
    uint32_t abiVersion;           /* RTGPU_ABI_VERSION */
    uint32_t numObjects;           /* traceable objects (shapes + finite lights) */
    uint32_t numTopNodes;          /* 0 when numObjects == 0 */
    uint32_t numLights;
    uint32_t numGlobalLights;
    uint32_t numMaterials;
    uint32_t numMeshes;
    uint32_t numMeshNodes;
    uint32_t numTriangles;
    uint32_t numVertices;
    uint32_t numTextures;
    uint32_t _pad;

    const RtNode*          topNodes;       /* [numTopNodes]  Scene::mTraceableObjectsBVH */
    const RtObject*        objects;        /* [numObjects]   */
    const RtLight*         lights;         /* [numLights]    Scene::mLights */
    const uint32_t*        globalLights;   /* [numGlobalLights] indices into lights[], Scene::mGlobalLights */
    const RtMaterial*      materials;      /* [numMaterials] */
    const RtMesh*          meshes;         /* [numMeshes]    */
    const RtNode*          meshNodes;      /* [numMeshNodes] */
    const RtTriangle*      triangles;      /* [numTriangles] */
    const RtVertexIndices* vertexIndices;  /* [numTriangles] */
    const RtVertexShading* vertexShading;  /* [numVertices]  */
    /* 128*128*4 uint16 = 131072 bytes, contents of Data/BlueNoise128_RGBA16.dat
     * (Core/Sampling/GenericSampler.cpp:13-52).  NULL => blue-noise dithering silently off (:72). */
    const uint16_t*        blueNoise;
    const RtTexture*       textures;       /* [numTextures] */
    const uint8_t*         texelData;      /* [texelBytes] rows of all bitmap textures (RtTexture::dataOffset points into it) */
    uint64_t               texelBytes;
} RtSceneDesc;

/* ---------------------------------------------------------------------------------------------
 * Per-pass constants: what Viewport::Render computes on the host before the tile fan-out
 * (Core/Rendering/Viewport.cpp:200-242) plus the RenderingParams fields the path reads
 * (Core/Rendering/Context.h:55-90) and the camera (Core/Scene/Camera.cpp:81-118).
 * ------------------------------------------------------------------------------------------- */

#define RTGPU_MAX_DIMENSIONS 4096u /* HaltonSequence::MaxDimensions */

typedef struct RtCamera
{
    float    localToWorld[16];   /* Camera::mLocalToWorld */
    float    aspectRatio;
    float    tanHalfFoV;         /* tanf(fov/2) computed by the host (Camera.cpp:37) */
    uint32_t dofEnable;
    uint32_t bokehShape;         /* rt::BokehShape (Camera.h:21-28): 0 circle, 1 hexagon, 2 square (NGon and Texture are refused) */
    float    focalPlaneDistance;
    float    aperture;
    float    barrelDistortionConstFactor;      /* Camera.cpp:86-91: applied when the variable factor is not zero; its random */
    float    barrelDistortionVariableFactor;   /* draw (ctx.randomGenerator.GetFloat()) comes from the per-pixel generator    */
    float    worldToScreen[16];  /* Camera::mWorldToScreen as SetPerspective left it (Camera.cpp:39-48): read by the
                                  * bidirectional integrator only (Camera::WorldToFilm, Camera.cpp:120-134) */
} RtCamera;

typedef enum RtLightSampling { RT_LIGHT_SAMPLING_SINGLE = 0, RT_LIGHT_SAMPLING_ALL = 1 } RtLightSampling;

typedef struct RtPassParams
{
    RtCamera camera;
    const uint32_t* seed;          /* [numDimensions] HaltonSequence::GetInt(d), Viewport.cpp:200-205 */
    uint32_t numDimensions;        /* SamplingParams::dimensions */
    uint32_t useBlueNoise;         /* SamplingParams::useBlueNoiseDithering */
    float    sampleOffset[2];      /* GetFloatNormal2(u) * antiAliasingSpread, Viewport.cpp:235-242 */
    uint32_t passIndex;            /* mProgress.passesFinished; even => also accumulate secondary sum */
    uint32_t maxRayDepth;
    uint32_t minRussianRouletteDepth;
    uint32_t lightSamplingStrategy;/* RtLightSampling */
    float    lightSamplingWeight[4]; /* PathTracerMIS::mLightSamplingWeight */
    float    bsdfSamplingWeight[4];  /* PathTracerMIS::mBSDFSamplingWeight  */
    /* Key of the per-pixel fallback generator.  The reference draws light picks
     * (PathTracerMIS.cpp:136) and samples past numDimensions (GenericSampler.cpp:108) from a
     * PER-THREAD xoroshiro128+ whose consumption order depends on dynamic tile scheduling; here every
     * pixel owns a xoroshiro128+ stream seeded from (rngKey, x, y) so the result is schedule-free. */
    uint64_t rngKey[2];
} RtPassParams;

/* rt::RayTracingCounters (Core/Rendering/Counters.h:36-93), intersection counters always on. */
typedef struct RtCounters
{
    uint64_t numRays;            /* sum over paths of depth+1  (PathTracerMIS.cpp:412) -- THE metric */
    uint64_t numShadowRays;
    uint64_t numShadowRaysHit;   /* reference naming: shadow rays that reached the light */
    uint64_t numPrimaryRays;
    /* The next four count CLOSEST-HIT traversals only, like the reference: Scene::Traverse resets and appends
     * the local counters (Scene.cpp:223,242) while Scene::Traverse_Shadow does neither, so the tests done by
     * shadow rays never reach RayTracingCounters there. */
    uint64_t numRayBoxTests;
    uint64_t numPassedRayBoxTests;
    uint64_t numRayTriangleTests;
    uint64_t numPassedRayTriangleTests;
    /* additions used by the roofline model */
    uint64_t numMeshHits;        /* EvaluateIntersection on a mesh triangle */
    uint64_t numAnalyticHits;    /* EvaluateIntersection on sphere/box/rect (incl. area lights) */
    uint64_t numShadowRayBoxTests;      /* box tests done by shadow rays (not counted by the reference) */
    uint64_t numShadowRayTriangleTests; /* triangle tests done by shadow rays */
    uint64_t numRetracedRays;    /* rays the default traversal kernel of single-mesh scenes did not trust (runner-up hit within its tolerance, NaN slab tests) and
                                  * handed to the binary-tree kernel, which walks the reference's order (performance statistic) */
    uint64_t _reserved[3];
} RtCounters;

typedef struct RtgpuContext RtgpuContext;

/* Optional tile-interleaved ownership for multi-GPU: this context renders only pixels whose 64x64
 * tile index (row-major) satisfies tile % worldSize == rank.  Non-owned pixels of the sum buffers
 * stay zero, so a sum-reduction (or gather) over ranks reproduces the 1-GPU image bit-exactly. */
typedef struct RtgpuShard
{
    uint32_t rank;
    uint32_t worldSize;
} RtgpuShard;

/* --- lifetime --------------------------------------------------------------------------------*/
/* Creates a context on HIP device `deviceIndex` (one context = one device = one host thread at a time). */
int  rtgpu_create(int deviceIndex, RtgpuContext** outCtx);
/* One context over several devices of a node: what the reference's ThreadPool does with the tiles of a frame across the cores of a
 * machine (Viewport.cpp:244-262, ThreadPool.cpp:176-260).  The frame's 64x64 tiles are dealt round-robin to the devices (RtgpuShard),
 * the scene is replicated by rtgpu_upload_scene, rtgpu_render_pass queues the pass on every device asynchronously, and the read-back
 * calls (rtgpu_read_sum, rtgpu_get_device_sum, rtgpu_postprocess, rtgpu_compute_block_errors) first gather the peers' tiles into the
 * first device's buffers (a kernel that reads the peers' HBM over xGMI; hipMemcpyPeerAsync staging without peer access or with
 * RTGPU_MULTI_STAGED=1).  Results are bit-identical to a one-device context; counters are summed.  deviceIndices == NULL: the first
 * numDevices visible devices (0 = all).  An index may repeat (two shards on one device: how the path is tested on a 1-GPU box).
 * Unsupported on such a context: rtgpu_set_shard, RT_INTEGRATOR_VCM / _LIGHT_TRACER (they splat over the whole frame);
 * rtgpu_get_kernel_times reports the first device. */
int  rtgpu_create_multi(const int* deviceIndices, uint32_t numDevices, RtgpuContext** outCtx);
int  rtgpu_num_devices(RtgpuContext* ctx, uint32_t* outCount);
void rtgpu_destroy(RtgpuContext* ctx);
const char* rtgpu_last_error(void);
uint32_t rtgpu_abi_version(void);

/* --- scene: replaces Scene::BuildBVH's pointer graph; copies everything, host memory may be freed.
 *     May be called again on a live context.  The passes queued before the call (either integrator's) are submitted first and render the old
 *     scene.  A scene is checked before anything is freed: a refused one (RTGPU_ERR_INVALID_ARGUMENT / _UNSUPPORTED) leaves the old scene, its
 *     photons and the history of rtgpu_denoise_temporal as they were.  An accepted one drops those photons and that history and the update
 *     record of rtgpu_get_update_info, and picks walk and shading kernels anew (rtgpu_get_walk_info is that of a fresh context given the
 *     scene); it keeps the film and the counters as they stand (rtgpu_reset is the caller's), the frame size, shard and active blocks, the
 *     integrator and its settings, and rtgpu_set_guide_chain. */
int rtgpu_upload_scene(RtgpuContext* ctx, const RtSceneDesc* scene);

/* --- moving objects: what the reference's demo does when the selected object is dragged -- ISceneObject::SetTransform
 *     (Demo_UserInterface.cpp:659), then Scene::BuildBVH (:701), which rebuilds only the top-level tree over the objects' boxes; the mesh
 *     trees belong to the shapes.  rtgpu_update_objects replaces the object table, the top-level nodes and (optionally) the light table of
 *     the uploaded scene in place, and nothing else.
 *   contract   numObjects and numLights equal the uploaded scene's; previousIndex is a permutation of 0 .. numObjects - 1; objects[i] equals
 *              the device's objects[previousIndex[i]] in every field but transform and invTransform (kind, shape, both parameter vectors,
 *              material, mesh and light index; the padding words too); lights[k] equals the device's lights[k] in every field but its two
 *              matrices (lights are never reordered).  invTransform is the caller's, as in RtObject.
 *   errors     a NULL argument, an abiVersion mismatch, a violated contract, a malformed top-level tree (a child or a leaf's objects out of
 *              range, more nodes than a tree over numObjects leaves can have): RTGPU_ERR_INVALID_ARGUMENT; a leaf of more than 3 objects, or
 *              the new top-level depth plus the deepest mesh tree beyond the 64-entry stack: RTGPU_ERR_UNSUPPORTED; before
 *              rtgpu_upload_scene: RTGPU_ERR_NOT_READY.  A refused update leaves the scene on the device exactly as it was.
 *   ordering   as rtgpu_upload_scene: the queued passes are submitted and every lane, ray query and AOV call is waited for first, so passes
 *              queued before the call render the old scene and passes after it the new one.  A multi-device context updates every peer.
 *   refreshes  the device's object table, top-level nodes and light table; the stack need; the axis-parallel-sun flag (a directional light's
 *              direction lives in its transform); the 4-wide top level of a two-level scene (rebuilt on the host: it lies in a slab of its
 *              own behind the mesh levels, so a top level of another size moves nothing) and the per-object level table, permuted.  The
 *              photons of the bidirectional integrator are dropped: they show the old scene.  The history of rtgpu_denoise_temporal is kept, with each
 *              object's motion beside it ("Temporal accumulation that follows moving objects", below).
 *   keeps      mesh nodes, triangles, shading records, textures, materials, the mesh levels of the 4-wide trees, the 4-wide tree of a
 *              single-mesh scene (its one object only changes its transform), the traversal kernel chosen at upload and the scene class.
 *              Nothing whose size grows with the triangle count is read, rebuilt or copied: RtUpdateInfo::bytesUploaded states what was.
 * rtgpu_get_update_info: the last successful update since rtgpu_upload_scene (all zero before the first): bytes copied to one device,
 * updates so far, the depth of the new top-level tree and the RTGPU_WALK_* kernel that serves the scene. */
typedef struct RtSceneUpdate
{
    uint32_t abiVersion, numObjects, numTopNodes, numLights;
    const RtNode*   topNodes;       /* [numTopNodes] the rebuilt Scene::mTraceableObjectsBVH */
    const RtObject* objects;        /* [numObjects]  in the NEW leaf order */
    const uint32_t* previousIndex;  /* [numObjects]  objects[i] was objects[previousIndex[i]] of the scene as it stands on the device */
    const RtLight*  lights;         /* [numLights]   Scene::mLights order, or NULL: the lights are unchanged */
} RtSceneUpdate;
int rtgpu_update_objects(RtgpuContext* ctx, const RtSceneUpdate* update);
typedef struct RtUpdateInfo { uint64_t bytesUploaded; uint32_t numUpdates, topDepth; uint32_t walk; uint32_t _pad[3]; } RtUpdateInfo;   /* 32 bytes; _pad[0]: rtgpu_update_mesh calls so far (below) */
int rtgpu_get_update_info(RtgpuContext* ctx, RtUpdateInfo* out);

/* --- deforming meshes: a mesh whose vertices moved (a skinned character, cloth, an edited vertex) keeps its topology, so every table that depends on its
 *     positions is a box or a triangle record.  rtgpu_update_mesh takes the new positions (12 bytes per vertex) and refits those tables ON THE DEVICE.
 *   triangles  triangle t of the mesh, in the device's (leaf) order, with vertex indices i0, i1, i2: v0 = P[i0], edge1 = P[i1] - P[i0], edge2 = P[i2] - P[i0],
 *              each lane one float subtraction (MeshShape::Initialize's arithmetic).  Its box is Box(P[i0], P[i1], P[i2]) of Math.h -- Min(a, Min(b, c))
 *              with Min(a, b) = a < b ? a : b per lane, Max alike --, taken from the positions, never from v0 + edge.
 *   boxes      a leaf takes the box of its first triangle, joined with those of its further ones in order (Box(box0, box1) = Min(box0.min, box1.min), ...);
 *              an interior node takes Box(child0, child1).  Node 1, which the builder never writes, stays; childIndex and leaves are never written.
 *   gates      the exact box of every leaf, where the 4-wide walks read it.
 *   grid       the grid of the mesh's 4-wide level is the one an upload computes over the new root box (the root node is read back for it).
 *   4-wide     every child slot is re-quantised from its binary node's new box by the upload's rule (in double, with the same push-out loops); its reference,
 *              leaf count or empty mark is kept.  WHICH binary nodes share a 4-wide node is kept as uploaded: it was chosen by surface area then, any choice
 *              returns the same hits, and a fresh upload of the same vertices may choose differently (and walk faster after a large deformation).
 *   shading    with shading != NULL the three RtVertexShading of every triangle's record are rewritten; its material is kept.  NULL: normals, tangents and
 *              texture coordinates stay.
 *   errors     a NULL argument, an abiVersion mismatch, flags != 0, meshIndex out of range, numVertices different from the mesh's, a position that is not
 *              finite or positions spanning more than a float holds: RTGPU_ERR_INVALID_ARGUMENT; a mesh whose uploaded tree is not an exact tree over all its
 *              triangles (a shared or unreachable node, a leaf's triangles out of range, a triangle in no leaf or in two), or -- where the mesh has a 4-wide
 *              level -- new positions whose box the 16-bit grid cannot hold with the half step of margin the walks rest on (base = min - 4 steps rounds back
 *              onto min: a mesh far from its local origin for its size, or flat at a coordinate that is not zero; an upload leaves such a mesh to the binary
 *              walk, an update keeps the walk and so refuses: upload the scene instead): RTGPU_ERR_UNSUPPORTED; before rtgpu_upload_scene: RTGPU_ERR_NOT_READY.  A mesh without
 *              triangles: RTGPU_OK, nothing done.  Every check is made on the host first: a refused update leaves the device exactly as it was.
 *   ordering   as rtgpu_update_objects: queued passes are submitted first and show the old mesh; lanes, ray queries and AOV calls are waited for.  A
 *              multi-device context updates every peer (never run on two devices so far).
 *   refreshes  the tables above; the level records of every object that uses the mesh (instances share one level: one refit serves all); the grid of a
 *              single-mesh scene.  The photons of the bidirectional integrator are dropped.  The history of rtgpu_denoise_temporal is kept: under
 *              rtgpu_set_deform_tracking pixels whose first hit lies on an object of the mesh are followed through the triangle records the mesh had ("Temporal
 *              accumulation that follows deforming meshes", below); without it they start anew (their object's prevId is 0xFFFFFFFF in the table the call
 *              builds).  All others reproject as before.
 *   keeps      topology, materials, textures, the scene class, the chosen walk, the top level and the object table: when the mesh's box changed, the caller
 *              follows with rtgpu_update_objects and a top-level tree over the new boxes (rtgpu_read_mesh tells the new root box).
 * rtgpu_get_update_info counts these calls in _pad[0]; bytesUploaded is that of the last update of either kind.
 * rtgpu_read_mesh: the mesh's nodes as they stand on the device, in the CALLER's node order and with the caller's child indices (nodes[numNodes]), and its
 * triangles (triangles[numTriangles]); either may be NULL.  rtgpu_read_wide_level: the 4-wide level that serves object objectIndex (object 0 of a
 * single-mesh scene) -- its WideLevel-shaped record (64 bytes: node base, gate base, triangle base, valid, grid base / step / bound), its raw 16-byte node
 * records and its gate records; nodeBytes / gateBytes are the buffers' sizes and must hold the level (info->pad[0] node records, info->pad[1] gate
 * records; call with NULL buffers to learn them).  RTGPU_ERR_NOT_READY for an object without such a level.  Both synchronise, as rtgpu_read_sum does. */
typedef struct RtMeshUpdate
{
    uint32_t abiVersion, meshIndex, numVertices, flags /* 0 */;
    const float*           positions;   /* [numVertices][3], mesh-local, the order of the VertexBufferDesc the mesh was made from */
    const RtVertexShading* shading;     /* [numVertices] or NULL: normals, tangents and texture coordinates stay */
} RtMeshUpdate;
int rtgpu_update_mesh(RtgpuContext* ctx, const RtMeshUpdate* update);
/* --- deforming meshes from device memory: what moves the vertices (skinning, cloth, a morph) usually runs on the same device.  rtgpu_update_mesh_device is
 *     rtgpu_update_mesh on arrays that are there already: no host copy of the positions, and the two checks that walk them are made by a kernel.
 *   semantics  exactly rtgpu_update_mesh's on the same values: the same tables bit for bit, the same ordering (queued passes first; lanes, ray queries and AOV
 *              calls waited for), the same effects on the photons, on the history of rtgpu_denoise_temporal and on the snapshot of
 *              rtgpu_set_deform_tracking, and the same count in RtUpdateInfo::_pad[0].  The two entries share one body from "the positions are in the mesh's
 *              device buffer" on.  bytesUploaded counts what crossed between host and device: the vertex indices and depth offsets with a mesh's first
 *              update, the root node read back and the level table of a two-level scene -- never the arrays.
 *   arrays     tight float3 arrays of numVertices entries in device memory of the context's device.  normals / tangents: either may be NULL, and then that
 *              half of every vertex record keeps what it holds; texture coordinates are never re-sent (a kernel rewrites the first 24 bytes -- or the 12
 *              given -- of each of the three 32-byte vertex records of a triangle, and leaves texCoord, the material and the padding alone).
 *   stream     the stream the caller produced the arrays on; NULL: the context's own.  The call orders itself behind that stream with an event, copies the
 *              arrays device to device into the mesh's own buffers and refits on the context's stream, as rtgpu_update_mesh does.  It returns synchronised
 *              (it reads the root box back anyway): the caller may overwrite or free the arrays on return.
 *   checks     before anything is launched, every given pointer is held to hipPointerGetAttributes and hipMemGetAddressRange: memory of the context's device,
 *              4-byte aligned, whose allocation holds 12 * numVertices bytes from the pointer on -- else RTGPU_ERR_INVALID_ARGUMENT: no kernel reads past an
 *              allocation.  Then one read-only kernel (k_refit_check) tells whether any of the 3 * numVertices floats is not finite and folds the box over the
 *              positions the triangles REFER to (a vertex no triangle uses does not count, as on the host), by atomic minimum and maximum over
 *              order-preserving keys of the floats: exact whatever the order of the blocks.  The host reads those 32 bytes and decides as rtgpu_update_mesh
 *              does, with the same statuses and messages; the box can differ from the host loop's only in the sign of a zero bound, which no decision
 *              depends on.  With a mesh's first update its vertex indices go to the device BEFORE the check (the kernel gathers through them): a private
 *              array that no walk reads, so "a refused update leaves the device exactly as it was" holds for everything a pass, a query or a read-back can see.
 *   errors     rtgpu_update_mesh's, and: a pointer that fails the checks above: RTGPU_ERR_INVALID_ARGUMENT; a multi-device context (the arrays live on one
 *              device): RTGPU_ERR_UNSUPPORTED -- rtgpu_update_mesh serves it.
 *   outBox     (may be NULL) min.xyz, max.xyz of the REFITTED ROOT NODE, read back after the refit -- the floats the host mirror's fold produces, bit for bit,
 *              zero signs included, never the check's box: what a top level over the new boxes is built from (rtgpu_update_objects follows, as above).
 *              Untouched where nothing was refitted (a mesh without triangles). */
typedef struct RtMeshUpdateDevice
{
    uint32_t abiVersion, meshIndex, numVertices, flags /* 0 */;
    const float* positions;   /* device, [numVertices][3] tight */
    const float* normals;     /* device, [numVertices][3] or NULL: stay */
    const float* tangents;    /* device, [numVertices][3] or NULL: stay */
} RtMeshUpdateDevice;
int rtgpu_update_mesh_device(RtgpuContext* ctx, const RtMeshUpdateDevice* update, void* stream, float outBox[6]);
/* The check alone, for tests and measurements: k_refit_check over `positions` (device, [numVertices][3], held to the pointer checks above) and the triangles of
 * mesh meshIndex, on `stream` (NULL: the context's own), into outRecord -- 32 bytes of device memory of the context's device: uint32 lo[3], hi[3] (keys of the box
 * over the referenced positions: key = bits ^ 0xFFFFFFFF for a negative float, bits | 0x80000000 otherwise; 0xFFFFFFFF / 0 where the mesh has no triangle),
 * nonFinite (blocks that met a float that is not finite), pad.  Asynchronous: it returns when the two launches are queued and writes no scene table.  The
 * mesh's vertex indices go to the device with the first call for a mesh, as with its first update. */
int rtgpu_refit_check_async(RtgpuContext* ctx, uint32_t meshIndex, uint32_t numVertices, const float* positions, void* outRecord, void* stream);
typedef struct RtWideLevelInfo { uint32_t nodeBase, gateBase, triBase, valid; float base[3], step[3], bound[3]; uint32_t pad[3]; } RtWideLevelInfo;   /* 64 bytes */
int rtgpu_read_mesh(RtgpuContext* ctx, uint32_t meshIndex, RtNode* nodes, RtTriangle* triangles);
int rtgpu_read_wide_level(RtgpuContext* ctx, uint32_t objectIndex, RtWideLevelInfo* info, void* nodes, uint64_t nodeBytes, void* gates, uint64_t gateBytes);

/* --- film: Viewport::Resize (Viewport.cpp:52-107) / Viewport::Reset (:120-138) ------------------
 * All three first submit every pass rtgpu_render_pass has queued -- the bidirectional integrator's batch included -- and wait for it: a queued
 * pass renders the film it was queued for (and counts in rtgpu_get_counters), never the one behind the call.
 *   rtgpu_resize     a new film of the given size, both sum buffers zero.  Drops the active blocks of rtgpu_set_active_blocks (the whole
 *                    image is active again), the photons of RT_INTEGRATOR_VCM (the next pass merges nothing) and the history of
 *                    rtgpu_denoise_temporal (the next such call starts every pixel), also when the size is the one the context has.  It alone
 *                    drops the ray source of rtgpu_set_ray_source or the lens source of rtgpu_set_lens_source too (the camera renders again); rtgpu_set_shard
 *                    and rtgpu_reset keep it.
 *                    Keeps the scene, the integrator and its settings, the shard, the counters, rtgpu_set_guide_chain, and whatever device
 *                    memory still suffices.  A refused size (0, or above 65536) changes nothing.
 *   rtgpu_set_shard  the same for a new ownership of the frame's tiles.
 *   rtgpu_reset      zeroes both sum buffers, the counters and the kernel times.  Keeps everything else, the active blocks and the history of
 *                    rtgpu_denoise_temporal included (a moving camera resets the film every frame); the bidirectional integrator starts over
 *                    with the pass whose passIndex is 0. */
int rtgpu_resize(RtgpuContext* ctx, uint32_t width, uint32_t height);
int rtgpu_set_shard(RtgpuContext* ctx, RtgpuShard shard);
int rtgpu_reset(RtgpuContext* ctx);

/* --- the hot path: one pass over every owned pixel (Viewport.cpp:244-262 -> RenderTile :291-357 ->
 *     PathTracerMIS::RenderPixel PathTracerMIS.cpp:254-415 -> Film::AccumulateColor Film.cpp:31-39).
 *     Asynchronous on the context's stream; the params (incl. seed[]) are copied before return. */
int rtgpu_render_pass(RtgpuContext* ctx, const RtPassParams* params);

/* Blocks until all queued passes have finished. */
int rtgpu_synchronize(RtgpuContext* ctx);

/* --- readback: Viewport::GetSumBuffer (R32G32B32_Float, tight stride; row y of the bitmap is film
 *     row H-1-y, Viewport.cpp:309,354).  sumRGB / secondaryRGB: width*height*3 floats, either may be
 *     NULL.  Synchronises. */
int rtgpu_read_sum(RtgpuContext* ctx, float* sumRGB, float* secondaryRGB);

/* Optional: page-locks (hipHostRegister) a host buffer the caller passes to rtgpu_read_sum / rtgpu_postprocess again and again, so
 * that the copies run at the PCIe link's rate (a 1080p float3 frame: ~0.6 ms instead of ~3 ms).  Unregister before freeing the
 * buffer.  RTGPU_ERR_NO_DEVICE / RTGPU_ERR_DEVICE when it cannot be done: the buffer then simply stays pageable. */
int rtgpu_host_register(RtgpuContext* ctx, void* ptr, size_t bytes);
int rtgpu_host_unregister(RtgpuContext* ctx, void* ptr);

/* Device pointers of the float3 sum buffers (for RCCL gather/reduce by the caller).  Synchronises first (and gathers, on a
 * multi-device context): the buffers hold every pass queued so far. */
int rtgpu_get_device_sum(RtgpuContext* ctx, void** sumDevice, void** secondaryDevice, size_t* numFloats);

/* Counters accumulated since the last rtgpu_reset (Viewport::GetCounters is per pass; callers
 * difference two reads).  Synchronises. */
int rtgpu_get_counters(RtgpuContext* ctx, RtCounters* out);

/* Box / triangle test counters (numRayBoxTests ... numShadowRayTriangleTests).  In the reference they exist only
 * under the compile-time switch RT_ENABLE_INTERSECTION_COUNTERS (Core/Config.h:4, off by default); here they are a
 * run-time switch, OFF by default like there (the environment variable RTGPU_INTERSECTION_COUNTERS=1 turns them on for
 * contexts created afterwards).  They are the counters of the REFERENCE'S walk: with the switch on, every ray walks the binary
 * tree in the reference's order (k_trace); with it off, single-mesh scenes walk the 4-wide collapse of the same tree
 * (k_trace_wide: same hits, another visiting order; RTGPU_WIDE=0 keeps the binary walk).  numRays / numShadowRays /
 * numShadowRaysHit / numPrimaryRays / hit counts are always maintained.  Synchronises. */
int rtgpu_set_intersection_counters(RtgpuContext* ctx, int enable);

/* ---------------------------------------------------------------------------------------------
 * Integrator selection.  RT_INTEGRATOR_PATH_TRACER_MIS (default) is rt::PathTracerMIS; RT_INTEGRATOR_VCM is
 * rt::VertexConnectionAndMerging (Core/Rendering/VertexConnectionAndMerging.cpp, renderer name "VCM"): per pixel one light
 * sub-path (light vertices connected to the camera -> film splats, photons recorded for the next pass) and one camera
 * sub-path (light hits, next event estimation, connections to the pixel's light vertices, merging with the previous pass's
 * photons through the hash grid of Core/Utils/HashGrid.h).  RtVcmParams carries the public knobs of the class
 * (VertexConnectionAndMerging.h:35-53) with the constructor's defaults (.cpp:53-71).  RtPassParams::maxRayDepth,
 * lightSamplingStrategy, the Russian-roulette depth and the two weights are ignored by VCM (the reference's class does not
 * read them); passIndex == 0 restarts the merging radius and drops the recorded photons (PreRender, .cpp:84-138).
 * The draws the reference takes from the per-thread generator come from a per-pixel generator keyed by
 * RtPassParams::rngKey; film splats are float atomics (their summation order is not defined -- in the reference neither).
 * VCM needs the whole frame on one device: shard {0, 1} and no active-block restriction.  Synchronises. */
typedef enum RtIntegrator
{
    RT_INTEGRATOR_PATH_TRACER_MIS = 0,
    RT_INTEGRATOR_VCM = 1,
    RT_INTEGRATOR_PATH_TRACER = 2,  /* rt::PathTracer ("Path Tracer", Core/Rendering/PathTracer.cpp): BSDF sampling only -- no next event
                                     * estimation, no MIS; lightSamplingStrategy and the two weights of RtPassParams are ignored */
    RT_INTEGRATOR_DEBUG = 3,        /* rt::DebugRenderer ("Debug", Core/Rendering/DebugRenderer.cpp): one colour per pixel from the primary
                                     * ray's first hit, selected by rtgpu_set_debug_rendering_mode (default: TriangleID) */
    RT_INTEGRATOR_LIGHT_TRACER = 4  /* rt::LightTracer ("Light Tracer", Core/Rendering/LightTracer.cpp): one light path per pixel, every vertex
                                     * below RtPassParams::maxRayDepth connected to the camera (film splats); same per-pixel generator
                                     * convention and whole-frame requirement as VCM */
} RtIntegrator;
/* rt::DebugRenderingMode (Core/Rendering/DebugRenderer.h:7-33; the four intersection-counter modes exist in the reference only under
 * RT_ENABLE_INTERSECTION_COUNTERS, which is off: their raw values per pixel are the cost planes of rtgpu_render_aovs, RT_AOV_BOX_TESTS ..
 * RT_AOV_TRIANGLE_TESTS_PASSED) */
typedef enum RtDebugRenderingMode
{
    RT_DEBUG_CAMERA_LIGHT = 0, RT_DEBUG_TRIANGLE_ID, RT_DEBUG_DEPTH, RT_DEBUG_POSITION, RT_DEBUG_NORMALS, RT_DEBUG_TANGENTS, RT_DEBUG_BITANGENTS,
    RT_DEBUG_TEXCOORDS, RT_DEBUG_BASE_COLOR, RT_DEBUG_EMISSION, RT_DEBUG_ROUGHNESS, RT_DEBUG_METALNESS, RT_DEBUG_IOR
} RtDebugRenderingMode;
typedef struct RtVcmParams
{
    uint32_t maxPathLength;            /* mMaxPathLength = 10 */
    uint32_t useVertexConnection;      /* mUseVertexConnection = true */
    uint32_t useVertexMerging;         /* mUseVertexMerging = true */
    float    initialMergingRadius;     /* 0.02 */
    float    minMergingRadius;         /* 0.02 */
    float    mergingRadiusMultiplier;  /* 1.0 */
    uint32_t _pad[2];
    float    bsdfSamplingWeight[4];        /* mBSDFSamplingWeight      = 1 */
    float    lightSamplingWeight[4];       /* mLightSamplingWeight     = 1 */
    float    vertexConnectingWeight[4];    /* mVertexConnectingWeight  = 1 */
    float    cameraConnectingWeight[4];    /* mCameraConnectingWeight  = 1 */
    float    vertexMergingWeight[4];       /* mVertexMergingWeight     = 1 */
} RtVcmParams;
#define RT_VCM_MAX_PATH_LENGTH 16u
/* Synchronises (the queued passes render with the integrator they were queued under) and drops the recorded photons, whatever the integrator;
 * film, counters, active blocks, the history of rtgpu_denoise_temporal and rtgpu_set_guide_chain stay.  Refused settings change nothing. */
int rtgpu_set_integrator(RtgpuContext* ctx, uint32_t integrator, const RtVcmParams* vcm /* NULL: defaults */);
/* DebugRenderer::mRenderingMode; needs RT_INTEGRATOR_DEBUG.  Synchronises. */
int rtgpu_set_debug_rendering_mode(RtgpuContext* ctx, uint32_t mode);
/* number of photons recorded by the last VCM pass (the merge set of the next one).  Synchronises. */
int rtgpu_vcm_num_photons(RtgpuContext* ctx, uint32_t* outCount);

/* Batch lanes (1..6, default 4).  rtgpu_render_pass gathers passes into batches; consecutive batches run on
 * alternating HIP streams with their own path-state arenas, so the drain of one batch's traversal launches (a few
 * very long rays) overlaps with the next batch's kernels.  The film is still summed in pass order.  Performance
 * only: results do not depend on it.  1 = strictly serial kernels (what per-kernel timing wants).  Synchronises.
 * Replaces the thread-pool width of the reference (RenderingParams::numThreads, Viewport.cpp:44-50). */
int rtgpu_set_concurrency(RtgpuContext* ctx, uint32_t lanes);

/* Launch-sequence knobs of the PathTracerMIS pipeline (round 4).  Performance only: results do not depend on them (the parity tests run
 * every setting against the oracle).  Synchronises.
 *   RTGPU_SCHEDULE_TAIL_BOUNCE   the bounce at which a batch with dense path state hands its remaining paths to the fused tail kernel
 *                                (k_tail, rt_tail.hip: trace + the reference's own walk + shade in one persistent launch, per block);
 *                                0 = never, -1 = the library's policy (frames under 700 k owned pixels: bounce 6, else never).
 *   RTGPU_SCHEDULE_LOCAL_RETRACE 1 = a block of the 4-wide walks traces the rays it does not decide itself instead of handing them to a
 *                                launch of their own, 0 = never, -1 = the library's policy (frames under 400 k owned pixels). */
enum { RTGPU_SCHEDULE_TAIL_BOUNCE = 0, RTGPU_SCHEDULE_LOCAL_RETRACE = 1 };
int rtgpu_set_schedule(RtgpuContext* ctx, uint32_t knob, int32_t value);

/* ---------------------------------------------------------------------------------------------
 * Post-processing of the sum buffer into the displayable front buffer: Viewport::PostProcessTile
 * (Core/Rendering/Viewport.cpp:495-550) per pixel -- scale by 1 / numPasses, saturation, contrast as
 * FastExp(FastLog(c) * contrast), exposure and colour filter, tone mapping (Core/Color/ColorHelpers.h:78-132),
 * dithering, Vector4::ToBGR().  Bloom (bloomFactor > 0): the five blurred copies of the sum buffer of
 * Viewport::PerformPostProcess (:432-452; Bitmap::GaussianBlur, Core/Utils/Bitmap.cpp:880-1020, sigma = 2 * 2.5^i, 8 box
 * blurs per direction as running sums in the reference's order) are rebuilt from the current sum buffer by every call and
 * mixed in as PostProcessTile does (:512-524).  The reference's blur reads and writes out of bounds unless the width is a
 * multiple of 4, both sizes are <= 4096 and > 195 (its widest window): other sizes return RTGPU_ERR_UNSUPPORTED with
 * bloomFactor > 0.  Dithering uses a per-pixel hash of (x, y, ditherSeed) instead of the reference's
 * per-thread generator (which makes the reference's own front buffer thread-schedule dependent).
 * --------------------------------------------------------------------------------------------- */
typedef enum RtTonemapper { RT_TONEMAPPER_CLAMPED = 0, RT_TONEMAPPER_REINHARD = 1, RT_TONEMAPPER_HEJL_BURGESS_DAWSON = 2, RT_TONEMAPPER_ACES = 3 } RtTonemapper;

typedef struct RtPostprocessParams   /* PostprocessParams, Core/Rendering/PostProcess.h:10-28 (defaults: PostProcess.cpp:6-14) */
{
    float    colorFilter[4];
    float    exposure;            /* log2 scale: colorScale = colorFilter * 2^exposure (Viewport.cpp:455) */
    float    contrast;
    float    saturation;
    float    ditheringStrength;
    float    bloomFactor;         /* PostprocessParams::bloomFactor (0 = off) */
    uint32_t tonemapper;          /* RtTonemapper */
    uint32_t numPasses;           /* pixelScaling = 1 / numPasses (1 + passesFinished at the time of the call, :502) */
    uint32_t ditherSeed;
} RtPostprocessParams;

/* frontBufferBGRA: host, width * height uint32 (0x00RRGGBB), row y = sum-buffer row y.  Synchronises. */
int rtgpu_postprocess(RtgpuContext* ctx, const RtPostprocessParams* params, uint32_t* frontBufferBGRA);

/* ---------------------------------------------------------------------------------------------
 * Adaptive rendering support (Viewport::ComputeBlockError / UpdateBlocksList, Core/Rendering/Viewport.cpp:552-700).
 * The block list lives on the host (the mirror's rt::Viewport keeps the reference's splitting logic); the device
 * computes the error estimates and restricts the passes to the pixels of the active blocks.
 * --------------------------------------------------------------------------------------------- */
typedef struct RtBlock { uint32_t minX, maxX, minY, maxY; } RtBlock;   /* Block: [minX, maxX) x [minY, maxY) in sum-buffer coordinates */

/* outErrors[i] = Viewport::ComputeBlockError(blocks[i]) with imageScalingFactor = 1 / numPasses: per pixel
 * (|a-b|.x + 2 |a-b|.y + |a-b|.z) / sqrt(RT_EPSILON + a.x + 2 a.y + a.z), a = sum / n, b = 2 secondarySum / n, summed
 * row by row in the reference's order, times sqrt(blockArea / imageArea) / blockArea.  Synchronises. */
int rtgpu_compute_block_errors(RtgpuContext* ctx, uint32_t numPasses, uint32_t numBlocks, const RtBlock* blocks, float* outErrors);

/* Restricts the following passes to the pixels covered by the blocks (intersected with the shard's tiles);
 * numBlocks = 0 restores the whole image.  Blocks must not overlap.  Synchronises. */
int rtgpu_set_active_blocks(RtgpuContext* ctx, uint32_t numBlocks, const RtBlock* blocks);

/* Evaluates textures of the uploaded scene on the device: out[4*i..] = ITexture::Evaluate(textures[textureIndex[i]],
 * (uv[2*i], uv[2*i+1])).  Host pointers; synchronous.  Exists so that the device decode of every texel format can be
 * checked against the reference's vectors directly (tests/golden/texture_kat.bin). */
int rtgpu_evaluate_textures(RtgpuContext* ctx, uint32_t count, const uint32_t* textureIndex, const float* uv, float* out);

/* ---------------------------------------------------------------------------------------------
 * Batched ray queries: Scene::Traverse (Core/Scene/Scene.h:56), Scene::Traverse_Shadow (:60) and Scene::EvaluateIntersection (:62) of the
 * uploaded scene.  Closest-hit rays take the walk the context renders with (the 4-wide walks and their re-trace hand-over by default; the
 * reference's binary walk under rtgpu_set_intersection_counters(ctx, 1)) from +inf, and maxDistance is applied to the result; any-hit rays take
 * the reference's binary walk with tmax = maxDistance (the 4-wide walks' any-hit decision is not exact for a tmax within an ulp of a hit).
 *   ray        Ray(origin, direction) as the reference's constructor builds it: the direction is normalised and distances are measured along
 *              it; no origin offset is applied (offsetting is the caller's job).
 *   RTGPU_TRACE_CLOSEST  hits[i] = Scene::Traverse with hitPoint.distance = maxDistance (+inf allowed).  Miss: objectId RT_INVALID_OBJECT,
 *              distance = maxDistance, subObjectId = u = v = 0.  A finite light: subObjectId RT_LIGHT_OBJECT.  u, v are the barycentrics of a mesh
 *              triangle; 0 on analytic shapes and lights.  surfaces (may be NULL) = Scene::EvaluateIntersection of the hit, normal mapping
 *              included; on a miss all zeros with material RT_NO_MATERIAL.
 *   RTGPU_TRACE_ANY      occluded[i] = Scene::Traverse_Shadow with hitPoint.distance = maxDistance, 1 or 0 (no offset: the Light Tracer's 0).
 *   degenerate rays      a non-finite origin, a zero or non-finite direction (its squared length 0 or not finite), or maxDistance NaN or <= 0:
 *              closest -> a miss (distance = maxDistance), any -> 0, never an undefined memory access.  rtgpu_trace_rays refuses a call that
 *              holds one (RTGPU_ERR_INVALID_ARGUMENT); rtgpu_trace_rays_async cannot inspect device memory, and the result rule holds there.
 *   stats      (may be NULL) the query's own counters, counted as the render counters are (box / triangle tests with the intersection counters
 *              on: closest-hit tests -- those of the walk from +inf -- in numRay*Tests, any-hit tests in numShadowRay*Tests; numRays = the call's
 *              closest-hit rays; numMeshHits / numAnalyticHits = evaluated surfaces).  A query never adds to what rtgpu_get_counters reports.
 *   errors     count == 0 is a no-op; NULL buffers with count > 0, an unknown mode, hits / surfaces with RTGPU_TRACE_ANY or occluded with
 *              RTGPU_TRACE_CLOSEST: RTGPU_ERR_INVALID_ARGUMENT; before rtgpu_upload_scene: RTGPU_ERR_NOT_READY.
 * Queries have their own path-state arena (176 bytes per ray, grown on first use up to a chunk of 4 M rays; larger calls run chunk by chunk),
 * queues and counters, and leave the render state alone.  A multi-device context (rtgpu_create_multi) answers on its first device.
 * --------------------------------------------------------------------------------------------- */
#define RTGPU_TRACE_CLOSEST 0u
#define RTGPU_TRACE_ANY     1u

/* 32 bytes (two 16-byte loads) */
typedef struct RtQueryRay
{
    float origin[3];
    float maxDistance;
    float direction[3];
    float _pad;
} RtQueryRay;

/* 32 bytes: rt::HitPoint (Core/Traversal/HitPoint.h) and three padding words (two 16-byte stores) */
typedef struct RtQueryHit
{
    float    distance;
    uint32_t objectId;
    uint32_t subObjectId;
    float    u, v;
    uint32_t _pad[3];
} RtQueryHit;

/* 48 bytes: what Scene::EvaluateIntersection leaves in IntersectionData -- position = frame[3], normal = frame[2], tangent = frame[0]
 * (world space), texCoord.xy and the material index */
typedef struct RtQuerySurface
{
    float    position[3];
    float    normal[3];
    float    tangent[3];
    float    texCoord[2];
    uint32_t material;
} RtQuerySurface;

/* Host pointers; synchronous (flushes the queued passes first, as rtgpu_read_sum does). */
int rtgpu_trace_rays(RtgpuContext* ctx, uint32_t mode, const RtQueryRay* rays, uint32_t count, RtQueryHit* hits, RtQuerySurface* surfaces,
                     uint32_t* occluded, RtCounters* stats);
/* Device pointers (rays, hits and surfaces 16-byte aligned, stats a device RtCounters) on `stream` (a hipStream_t; NULL: the context's own
 * stream): ordered after the work already queued there, returns without synchronising. */
int rtgpu_trace_rays_async(RtgpuContext* ctx, uint32_t mode, const RtQueryRay* rays, uint32_t count, RtQueryHit* hits, RtQuerySurface* surfaces,
                           uint32_t* occluded, RtCounters* stats, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Path records: the reference's PathDebugData hook (Core/Rendering/PathDebugging.h:27-53, filled by PathTracerMIS::RenderPixel at
 * PathTracerMIS.cpp:377-410; its Demo draws the picked pixel's path from it).  For each pixel (x, y) -- sum-buffer coordinates, as in
 * RtBlock; the film row flips inside -- the call traces the path rtgpu_render_pass(ctx, params) would trace for it on this context and
 * writes its vertices in path order: one per vertex the path goes on from, with the sampled BSDF event, and a closing one where it ends.
 *   RtPathVertex  28 words: 0-2 ray origin, 3-5 ray direction, 6 objectId, 7 subObjectId (uint32), 8 distance, 9-10 u v, 11-13 position,
 *              14-16 normal, 17-19 tangent (the evaluated frame, world space), 20-21 texCoord, 22-25 throughput, 26 bsdfEvent (uint32), 27 zero.
 *              Zero where the reference leaves what an earlier vertex wrote (one HitPoint and one ShadingData live for its whole path):
 *              on a miss word 7 and words 9..21; on a hit that is not a mesh triangle words 9 and 10; word 26 of the closing record.
 *   RtPathInfo    numVertices = the path's count; only the first maxVertices are stored, and of a pixel's maxVertices entries in `vertices`
 *              only those the path has are written.  terminationReason = PathTerminationReason, set at the branches of PathTracerMIS.cpp:
 *              280-367.  radiance = what the pass would add to the pixel.
 *   errors     numPixels == 0 is a no-op; NULL buffers with numPixels > 0, a pixel outside the frame, maxVertices == 0 and what
 *              rtgpu_render_pass refuses in the params: RTGPU_ERR_INVALID_ARGUMENT (and its RTGPU_ERR_UNSUPPORTED); before
 *              rtgpu_upload_scene / rtgpu_resize: RTGPU_ERR_NOT_READY; any integrator but RT_INTEGRATOR_PATH_TRACER_MIS: RTGPU_ERR_UNSUPPORTED.
 * Host pointers; synchronous (flushes the queued passes first).  A pixel may repeat; shards and active blocks do not restrict the call, and a
 * multi-device context answers on its first device.  It traces with the walk the context renders with, on an arena, queues and counters of
 * its own (sized by numPixels, grown on use, freed with the context), is not a pass, and leaves film, sum buffers, counters and kernel
 * times alone.
 * --------------------------------------------------------------------------------------------- */
typedef enum RtPathTerminationReason
{
    RT_PATH_HIT_BACKGROUND = 1, RT_PATH_HIT_LIGHT = 2, RT_PATH_DEPTH = 3, RT_PATH_THROUGHPUT = 4, RT_PATH_NO_SAMPLED_EVENT = 5, RT_PATH_RUSSIAN_ROULETTE = 6
} RtPathTerminationReason;
typedef struct RtPathVertex { float w[28]; } RtPathVertex;   /* 112 bytes */
typedef struct RtPathInfo { uint32_t numVertices, terminationReason; float radiance[3]; uint32_t _pad[3]; } RtPathInfo;   /* 32 bytes */
int rtgpu_record_paths(RtgpuContext* ctx, const RtPassParams* params, const uint32_t* pixelsXY /* 2 per pixel */, uint32_t numPixels,
                       uint32_t maxVertices, RtPathVertex* vertices /* [numPixels * maxVertices] */, RtPathInfo* infos /* [numPixels] */);

/* ---------------------------------------------------------------------------------------------
 * AOVs: what the primary ray of every pixel finds, as raw planes in one call -- first-hit geometry, the evaluated material and the cost of
 * the traversal.  For every pixel of the frame the call generates the primary ray rtgpu_render_pass(ctx, params) would generate for it (the
 * same sampler draws: depth of field, bokeh, barrel distortion), traces it (Scene::Traverse from +inf) and evaluates
 * Scene::EvaluateIntersection and Material::EvaluateShadingData at the hit -- the values the debug modes (RtDebugRenderingMode) squeeze into
 * a display colour, unsqueezed.
 *   layout     outputs[k] receives plane planes[k] channel-major: channels x height x width 32-bit words (a (C, H, W) tensor); row y is
 *              sum-buffer row y, as in RtBlock (the film row flips inside).
 *   values     on a miss everything is 0 except DEPTH (+inf), OBJECT_ID (RT_INVALID_OBJECT) and MATERIAL (RT_NO_MATERIAL).  On a finite
 *              light the geometry planes hold what Scene::EvaluateIntersection returns, the material planes 0 and MATERIAL RT_NO_MATERIAL.
 *              The four cost planes are the reference's ctx.localCounters after that one Traverse, counted as RtCounters::numRayBoxTests ..
 *              numPassedRayTriangleTests are (they walk the reference's binary tree whatever the context renders with; without them the
 *              call takes the walk the context renders with).
 *   errors     numPlanes == 0 is a no-op; NULL arguments with numPlanes > 0, a plane id >= RT_AOV_NUM_PLANES or the same plane twice:
 *              RTGPU_ERR_INVALID_ARGUMENT; what rtgpu_render_pass refuses in the params gets the status it gets there; before
 *              rtgpu_upload_scene / rtgpu_resize: RTGPU_ERR_NOT_READY.
 * It submits the passes queued on the device it answers on first, is not a pass, and leaves film, sum buffers, counters, kernel times and the photon state alone.  It
 * works whichever integrator is selected; shards and active blocks do not restrict it, and a multi-device context answers on its first
 * device.  Arena and queues are its own (grown on use, freed with the context); a chunk holds at most 4 M pixels (RTGPU_AOV_CHUNK),
 * larger frames run chunk by chunk.
 * --------------------------------------------------------------------------------------------- */
typedef enum RtAovPlane {            /* words per pixel, type */
    RT_AOV_DEPTH = 0,                /* 1 f32  HitPoint::distance; +inf on a miss            */
    RT_AOV_POSITION,                 /* 3 f32  frame[3]                                      */
    RT_AOV_NORMAL,                   /* 3 f32  frame[2] (normal map applied)                 */
    RT_AOV_TANGENT,                  /* 3 f32  frame[0]                                      */
    RT_AOV_BITANGENT,                /* 3 f32  frame[1]                                      */
    RT_AOV_TEXCOORD,                 /* 2 f32                                                */
    RT_AOV_BARYCENTRICS,             /* 2 f32  HitPoint u, v (0 off mesh triangles)          */
    RT_AOV_BASE_COLOR,               /* 3 f32  ShadingData::materialParams after textures    */
    RT_AOV_EMISSION,                 /* 3 f32                                                */
    RT_AOV_ROUGHNESS, RT_AOV_METALNESS, RT_AOV_IOR,   /* 1 f32 each                          */
    RT_AOV_OBJECT_ID,                /* 1 u32  RT_INVALID_OBJECT on a miss                   */
    RT_AOV_SUB_OBJECT_ID,            /* 1 u32  triangle; RT_LIGHT_OBJECT on a finite light   */
    RT_AOV_MATERIAL,                 /* 1 u32  global material index; RT_NO_MATERIAL on a miss or a light */
    RT_AOV_BOX_TESTS, RT_AOV_BOX_TESTS_PASSED, RT_AOV_TRIANGLE_TESTS, RT_AOV_TRIANGLE_TESTS_PASSED,  /* 1 u32 each */
    RT_AOV_NUM_PLANES
} RtAovPlane;
/* Host pointers; synchronous. */
int rtgpu_render_aovs(RtgpuContext* ctx, const RtPassParams* params, const uint32_t* planes, uint32_t numPlanes, void* const* outputs);
/* Device pointers (16-byte aligned) on `stream` (a hipStream_t; NULL: the context's own stream): ordered after the work already queued
 * there, returns without synchronising.  `planes`, `outputs` and `params` themselves are host memory and may be reused on return. */
int rtgpu_render_aovs_async(RtgpuContext* ctx, const RtPassParams* params, const uint32_t* planes, uint32_t numPlanes, void* const* outputs,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * Guide chains: the AOV planes at the first vertex of a pixel's path that is not a mirror or a pane of glass.  Inside a reflection the first
 * hit is the wrong surface to steer a filter by: the mirror's normal, position and base colour are constant over the whole reflected scene.
 * The chain call follows the pixel's path through such surfaces and evaluates the planes where it stops.
 *   the path   For a pixel, the path RT_INTEGRATOR_PATH_TRACER_MIS would trace for it under `params`, whichever integrator the context has
 *              selected: the same sampler draws in the same order.  At every surface vertex these are the next-event draws of the pass's
 *              light-sampling mode (RT_LIGHT_SAMPLING_SINGLE: the light pick when the scene has more than one light, then three floats;
 *              RT_LIGHT_SAMPLING_ALL: three floats per light; none in a scene without lights), the roulette draw from
 *              minRussianRouletteDepth on, and the three BSDF draws.
 *   passed     Vertex j (j = depth, from 0) is PASSED iff all of these hold:
 *                - the path goes on from it: it is not the closing vertex (not a miss, not a finite light, not ended by maxRayDepth,
 *                  roulette, a zero throughput or a missing BSDF event);
 *                - its sampled event is specular (RtPathVertex::bsdfEvent & 48: specular reflection 16 or specular refraction 32);
 *                - its material's bsdf is RT_BSDF_DIELECTRIC, RT_BSDF_ROUGH_DIELECTRIC, RT_BSDF_METAL or RT_BSDF_ROUGH_METAL;
 *                - j < maxChain.
 *              The (bsdf, roughness) pairs that can return a specular event at all: DIELECTRIC and METAL at any roughness; ROUGH_DIELECTRIC,
 *              ROUGH_METAL, ROUGH_PLASTIC with an evaluated roughness < 0.005 (below it they sample as their smooth siblings); PLASTIC at any
 *              roughness.  PLASTIC and ROUGH_PLASTIC are excluded on purpose: the coat samples a specular event with probability >= 0.25
 *              at every vertex, and following it would salt a plastic floor with reflection guides pixel by pixel.
 *   the guide  The GUIDE VERTEX is vertex k, the first one not passed.
 *   planes     - the 15 non-cost planes of RtAovPlane (DEPTH .. MATERIAL) mean what they mean for rtgpu_render_aovs, evaluated at the guide
 *                vertex with that vertex's own ray: a secondary ray is Ray(origin, direction) with the origin then moved by direction * 0.001f.
 *                DEPTH is that ray's hit distance, +inf on a miss.  On a miss everything else is 0 except OBJECT_ID (RT_INVALID_OBJECT) and
 *                MATERIAL (RT_NO_MATERIAL); on a finite light the geometry planes hold what Scene::EvaluateIntersection returns -- at
 *                depth > 0 with the previous vertex's material still in IntersectionData::material, so that material's normal map (if any)
 *                is applied to the light's frame, as the reference's path tracer does -- the material planes are 0 and MATERIAL is
 *                RT_NO_MATERIAL.  BARYCENTRICS are non-zero on mesh triangles only.
 *              - RT_AOV_CHAIN_LENGTH     1 u32  k
 *              - RT_AOV_CHAIN_DISTANCE   1 f32  ((d_0 + d_1) + ...) + d_k, the hit distances of vertices 0..k summed left to right in f32;
 *                                               +inf when the guide vertex is a miss
 *              - RT_AOV_CHAIN_THROUGHPUT 3 f32  the path throughput on arrival at the guide vertex: 1 for k = 0, otherwise what vertex k - 1
 *                                               leaves behind (BSDF value over pdf, roulette division included)
 *              - the four cost planes (RT_AOV_BOX_TESTS .. RT_AOV_TRIANGLE_TESTS_PASSED) are refused: they describe one traversal.
 *   bounds     params->maxRayDepth and minRussianRouletteDepth bound the chain as they bound the path.  A caller who wants chains that
 *              roulette never cuts passes guide params with minRussianRouletteDepth >= maxChain.
 *   identity   maxChain == 0 gives the bits of rtgpu_render_aovs on every common plane.
 *   errors     those of rtgpu_render_aovs; chain NULL, maxChain > RT_AOV_CHAIN_MAX, non-zero flags, or a cost plane:
 *              RTGPU_ERR_INVALID_ARGUMENT.  The chain plane ids lie behind RT_AOV_NUM_PLANES: rtgpu_render_aovs refuses them.
 * Layout, stream, alignment, chunking (RTGPU_AOV_CHUNK), multi-device, shard and active-block rules are those of rtgpu_render_aovs[_async].
 * The calls submit the passes queued on the device they answer on first, are not passes, and leave film, sum buffers, counters, kernel times,
 * the photon state, the path recorder and the temporal history alone.  Arena and queues are their own, grown on use, freed with the context.
 * A vertex whose material cannot pass, or whose depth is maxChain, stops before a draw is taken: a frame without mirrors and glass costs
 * what the first-hit call costs plus one shading launch that evaluates the hit.
 *
 * rtgpu_set_guide_chain makes rtgpu_denoise[_async] and rtgpu_denoise_var[_async] render their DEPTH, NORMAL, POSITION and BASE_COLOR guides
 * through the chain call: by definition the result is rtgpu_render_aovs_chain followed by the pure filter entry on the same planes.  NULL
 * clears it (first hit, the default).  While a chain is set, rtgpu_denoise_temporal* and rtgpu_denoise_temporal_clip* answer
 * RTGPU_ERR_UNSUPPORTED and leave the history as it was.
 * Measured (one MI355X, Sponza-class 1920 x 1080, maxChain 3; tools/bench_aovs.py and tools/bench_denoise.py with --chain 3 --mirror): the four
 * guide planes take 0.93 ms against the first-hit call's 0.57 where nothing is specular, 1.82 against 0.74 with a mirror and a glass sphere over a sixth of the frame.
 * At 16 passes the plain filter's relative MSE inside the mirror is 0.187 with chain guides against 0.216 without; under the variance-guided filter chain guides
 * measure worse (mirror 0.088 against 0.029, glass sphere 1.78 against 0.035).
 * Scope: temporal reprojection through a chain needs the virtual motion of the mirrored point: rtgpu_render_aovs_virtual and
 * rtgpu_denoise_temporal_chain (below) provide it, taking their chain as an argument; the entries under rtgpu_set_guide_chain still refuse.  On glass one
 * pass's guides pick reflect or refract per pixel by the pass's own draw while the colour averages both; a deterministic choice is not provided, so on glass
 * per-pixel chain lengths differ from frame to frame and most glass pixels start in the chained temporal call.
 * --------------------------------------------------------------------------------------------- */
#define RT_AOV_CHAIN_MAX 16u
typedef enum RtAovChainPlane {
    RT_AOV_CHAIN_LENGTH = RT_AOV_NUM_PLANES,   /* 1 u32 */
    RT_AOV_CHAIN_DISTANCE,                     /* 1 f32 */
    RT_AOV_CHAIN_THROUGHPUT,                   /* 3 f32 */
    RT_AOV_CHAIN_NUM_PLANES
} RtAovChainPlane;
typedef struct RtAovChain { uint32_t maxChain; /* 0 .. 16 vertices passed at most */ uint32_t flags; /* 0 */ uint32_t _pad[2]; } RtAovChain;   /* 16 bytes */
/* Host pointers; synchronous. */
int rtgpu_render_aovs_chain(RtgpuContext* ctx, const RtPassParams* params, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes,
                            void* const* outputs);
/* Device pointers (16-byte aligned) on `stream`, as rtgpu_render_aovs_async. */
int rtgpu_render_aovs_chain_async(RtgpuContext* ctx, const RtPassParams* params, const RtAovChain* chain, const uint32_t* planes,
                                  uint32_t numPlanes, void* const* outputs, void* stream);
int rtgpu_set_guide_chain(RtgpuContext* ctx, const RtAovChain* chain /* NULL: first hit, the default */);

/* ---------------------------------------------------------------------------------------------
 * The virtual position: where the guide vertex of a chain appears to be.  A point seen through plane mirrors appears at its virtual image, which lies
 * on the primary ray at the unfolded path length and does not depend on the camera: projected through another camera it lands on the pixel where that
 * camera sees the same reflected surface point.  This is the point temporal accumulation reprojects inside a reflection (the next sections).
 * rtgpu_render_aovs_virtual[_async] are rtgpu_render_aovs_chain[_async] in every respect -- arguments, rules, errors, and the bits of every plane the
 * chain call knows -- and accept plane ids below RT_AOV_VIRTUAL_NUM_PLANES; the chain call keeps refusing RT_AOV_VIRTUAL_POSITION as unknown.
 *   RT_AOV_VIRTUAL_POSITION  3 f32.  For a pixel let o and w be the origin and the direction of its primary ray as generated (RtPathVertex words 0..2 and
 *              3..5 of vertex 0: lens sample and distortion included), k its RT_AOV_CHAIN_LENGTH and D its RT_AOV_CHAIN_DISTANCE.
 *                - D == +inf (the guide vertex is a miss): 0, 0, 0, as POSITION is.
 *                - k == 0: the words of the POSITION plane.
 *                - otherwise, per channel c:   V_c = o_c + w_c * D   -- the multiply rounded, then the add rounded, never fused.
 *   scope      exact for any number of plane mirrors.  Behind a curved mirror or a refraction it is an approximation of where the surface appears; the
 *              per-tap surface test of temporal accumulation, run on the chain guides, is what catches the cases where it fails.
 * --------------------------------------------------------------------------------------------- */
typedef enum RtAovVirtualPlane {
    RT_AOV_VIRTUAL_POSITION = RT_AOV_CHAIN_NUM_PLANES,   /* 3 f32 */
    RT_AOV_VIRTUAL_NUM_PLANES
} RtAovVirtualPlane;
/* Host pointers; synchronous. */
int rtgpu_render_aovs_virtual(RtgpuContext* ctx, const RtPassParams* params, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes,
                              void* const* outputs);
/* Device pointers (16-byte aligned) on `stream`, as rtgpu_render_aovs_async. */
int rtgpu_render_aovs_virtual_async(RtgpuContext* ctx, const RtPassParams* params, const RtAovChain* chain, const uint32_t* planes,
                                    uint32_t numPlanes, void* const* outputs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The ray source: passes along caller-supplied primary rays.  Every image starts at Camera::GenerateRay (Core/Scene/Camera.cpp:81-118), a perspective
 * camera with a thin lens and barrel distortion.  A ray source replaces it at the source: a per-pixel table of primary rays -- an orthographic view, a
 * panorama, a calibrated lens, the rays that leave a lightmap texel -- from which rtgpu_render_pass and every call that follows a pass's primary rays
 * start.  Nothing behind the primary ray changes: the path records hold an origin and an unnormalised direction whoever wrote them.
 *   table      width * height entries of 32 bytes in sum-buffer coordinates, row-major (as in RtBlock and the AOV planes; the film row flips inside):
 *              entry y * width + x is the primary ray of pixel (x, y).  RtPrimaryRay has RtQueryRay's layout, so one buffer serves this call and
 *              rtgpu_trace_rays; words 3 and 7 are never read.  The direction need not be unit length: it goes into the path's direction record as
 *              given and Ray() normalises it wherever a ray is built -- rtgpu_trace_rays' rule, and the state in which the camera's direction is
 *              stored.  No origin offset is applied.
 *   while set  rtgpu_render_pass under RT_INTEGRATOR_PATH_TRACER_MIS, _PATH_TRACER and _DEBUG takes every pixel's primary ray from the table.
 *              RtPassParams::camera and sampleOffset are not read (nor checked).  The sampler and the per-pixel generator start as
 *              ResetPixel(x, y) with the pass's rngKey leaves them: a table ray is the ray of a camera that draws nothing.  All else of the pass is what
 *              it was: seeds, passIndex and the secondary sum, depth, roulette, light sampling, the counters (numPrimaryRays included), shards, active
 *              blocks, batching over lanes, both path-state layouts and the fused tail.
 *   followers  every call documented as generating "the primary ray rtgpu_render_pass would generate" does so under a source too: rtgpu_render_aovs*, the
 *              chain and virtual-position variants, rtgpu_record_paths -- hence rtgpu_denoise and rtgpu_denoise_var, whose guides the AOV call renders.
 *              The rtgpu_denoise_temporal* entries refuse with RTGPU_ERR_UNSUPPORTED, as under a guide chain: a table has no worldToScreen to reproject
 *              through (the pure rtgpu_temporal_accumulate* entries take planes and are untouched).  A pass under RT_INTEGRATOR_VCM or _LIGHT_TRACER
 *              while a source is set: RTGPU_ERR_UNSUPPORTED (they splat through Camera::WorldToFilm).
 *   setting    the queued passes are submitted first and render what they were queued for; lanes, ray queries and AOV calls are waited for, as in
 *              rtgpu_update_objects.  The table is copied into memory of the context (the caller may free or overwrite it on return; both entries return
 *              synchronised), and the COPY is checked by one read-only kernel (k_ray_source_check) before the source is replaced: an entry is degenerate
 *              if a word of its origin or direction is not finite or its direction's squared length is 0 or not finite -- the degenerate-ray rule of
 *              the ray queries.  A degenerate entry: RTGPU_ERR_INVALID_ARGUMENT, and the previous source, or the camera, stays exactly as it was; nothing
 *              degenerate ever reaches a walk.
 *   errors     count != width * height: RTGPU_ERR_INVALID_ARGUMENT; before rtgpu_resize: RTGPU_ERR_NOT_READY; rays == NULL with count == 0 clears the
 *              source, also a lens source (the camera renders again), rays == NULL with any other count: RTGPU_ERR_INVALID_ARGUMENT.
 *   _device    `rays` is device memory, held to hipPointerGetAttributes and hipMemGetAddressRange as rtgpu_update_mesh_device holds its arrays (memory of
 *              the context's device, 4-byte aligned, whose allocation holds 32 * count bytes from the pointer on -- else RTGPU_ERR_INVALID_ARGUMENT); the
 *              call orders itself behind `stream` (NULL: the context's own) with an event and copies device to device.  A multi-device context:
 *              RTGPU_ERR_UNSUPPORTED -- rtgpu_set_ray_source serves it and replicates the table to every device.
 *   keeps      rtgpu_upload_scene, the update calls, rtgpu_reset, rtgpu_set_shard, rtgpu_set_active_blocks and rtgpu_set_integrator keep the source.
 *   drops      rtgpu_resize, also when the size is the one the context has (like the active blocks): a table is a frame's.
 *   rtgpu_get_ray_source   outCount = the entries of the source, 0: the camera.
 * Exporting the camera's rays: rtgpu_read_camera_rays[_async] write, for every pixel of the frame, what the generate kernel would store for `params` -- the
 * origin and the unnormalised direction, in the table's layout and order, words 3 and 7 zero.  Not a pass: film, counters and queued passes are untouched;
 * a multi-device context answers on its first device.  It is where a caller starts who wants the camera's rays with a lens model of their own on top, and
 * what makes the source checkable bit for bit: a table exported from a camera renders that camera's frame.  A camera that draws from the sampler (dofEnable,
 * or barrelDistortionVariableFactor != 0): RTGPU_ERR_UNSUPPORTED -- a table cannot carry the draws the camera took.  The export writes the camera's rays
 * whether or not a source is set.  Before rtgpu_resize: RTGPU_ERR_NOT_READY.  The _async entry takes device memory (16-byte aligned, held to the pointer
 * checks above) on `stream` (NULL: the context's own) and returns without synchronising.
 * --------------------------------------------------------------------------------------------- */
typedef struct RtPrimaryRay { float origin[3]; float _pad0; float direction[3]; float _pad1; } RtPrimaryRay;   /* 32 bytes */
int rtgpu_set_ray_source(RtgpuContext* ctx, const RtPrimaryRay* rays, uint64_t count);                        /* host pointer */
int rtgpu_set_ray_source_device(RtgpuContext* ctx, const RtPrimaryRay* rays, uint64_t count, void* stream);   /* device pointer */
int rtgpu_get_ray_source(RtgpuContext* ctx, uint64_t* outCount);                                              /* 0: the camera */
int rtgpu_read_camera_rays(RtgpuContext* ctx, const RtPassParams* params, RtPrimaryRay* out);                        /* host; synchronous */
int rtgpu_read_camera_rays_async(RtgpuContext* ctx, const RtPassParams* params, RtPrimaryRay* out, void* stream);    /* device */

/* ---------------------------------------------------------------------------------------------
 * The lens source: a table of RECIPES for a pass's primary ray.  A ray source holds one finished ray per pixel, so a new sub-pixel offset per pass means a
 * new table per pass (and every set call ends the batch in flight), and a thin lens, whose sample must come from the pass's sampler on the device, cannot be
 * expressed at all.  A lens source holds, per pixel, the ray, its footprint -- its first-order change per unit of RtPassParams::sampleOffset -- and a thin
 * lens; the generate kernels apply the pass's offset and take the lens sample from the pass's sampler exactly as Camera::GenerateRay does.  One table then
 * serves every pass of a batch, jittered and defocused.  It is a second setting beside the ray source, whose contract is untouched: one context holds one
 * source, setting either kind replaces the other, and rtgpu_set_ray_source(ctx, NULL, 0) clears both.
 *   entry      RtLensRay, 128 bytes, eight float4; entry y * width + x is sum-buffer pixel (x, y), the plain table's indexing and row order:
 *                quad 0   origin.xyz                          w: aperture
 *                quad 1   direction.xyz (not normalised)      w: focalDistance
 *                quad 2,3 dOrigin/dsx, dOrigin/dsy            w: not interpreted
 *                quad 4,5 dDirection/dsx, dDirection/dsy      w: not interpreted
 *                quad 6,7 lensU, lensV (the lens plane's axes; the library does not normalise them)   w: not interpreted
 *              sx, sy are RtPassParams::sampleOffset[0], [1] as the caller passes them.
 *   a pass's ray, operation by operation (tests/lens_source_ref.py is the same text in float32 NumPy; the jitter step is reproducible bit for bit):
 *     1 jitter if sx == 0 and sy == 0: origin and direction are the stored words, untouched (a -0.0 component survives: it decides the sign of 1 / dir).
 *              Otherwise, for each of the six components v of origin and direction with its derivatives dvdsx, dvdsy:
 *                  v' = fadd(fadd(v, fmul(sx, dvdsx)), fmul(sy, dvdsy))
 *              every fmul and fadd an IEEE float32 operation rounded to nearest even on its own; nothing is contracted into a fused multiply-add.
 *     2 lens   only if the source was set with lens = 1.  EVERY pixel draws sampler.getFloat() twice, whatever its aperture (as the camera does under
 *              dofEnable), u1 then u2, and runs the dofEnable branch of Camera::GenerateRay (Camera.cpp:104-114) -- the camera kernels' branch, operation
 *              for operation -- on the jittered ray:
 *                  focusPoint = fma(direction, focalDistance, origin)
 *                  bokeh      = bokehShape 0: the circle of SamplingHelpers::GetCircle(u1, u2); 1: (u1 * -1 + u2 * 0.5, u1 * 0 + u2 * 0.8660254) (the hexagon's
 *                               first rhombus); 2: (2 u1 - 1, 2 u2 - 1)
 *                  p          = bokeh * aperture
 *                  origin     = fma(p.y, lensV, fma(p.x, lensU, origin))
 *                  direction  = focusPoint - origin
 *              with lensU, lensV in the places of the camera transform's rows 0 and 1.  With lens = 0 nothing is drawn: the sampler starts as under the
 *              ray source.
 *     3 guard  the final ray is held to the degenerate-ray rule of the ray queries (a word of the origin not finite; the direction's squared length 0 or
 *              not finite) -- jitter may cancel a direction, focalDistance and the lens offset may cancel.  A degenerate final ray is replaced by the
 *              entry's stored origin and direction, which the set call checked; the draws stay taken.  No degenerate ray reaches a walk, whatever the offsets.
 *   while set  as under the ray source (passes under RT_INTEGRATOR_PATH_TRACER_MIS, _PATH_TRACER and _DEBUG, the followers rtgpu_render_aovs*, the chain and
 *              virtual variants, rtgpu_record_paths, rtgpu_denoise and rtgpu_denoise_var; the same refusals: rtgpu_denoise_temporal*, RT_INTEGRATOR_VCM and
 *              _LIGHT_TRACER answer RTGPU_ERR_UNSUPPORTED), except that sampleOffset IS read: a sampleOffset that is not finite: RTGPU_ERR_INVALID_ARGUMENT.
 *              RtPassParams::camera is still neither read nor checked.
 *   setting    the ray source's life cycle: queued passes are submitted first, lanes, queries and AOV calls are waited for, the table is copied into the
 *              context's second buffer (128 * width * height bytes each, allocated once per frame size, dropped by rtgpu_resize and with the context) and
 *              checked there by one read-only kernel (k_lens_source_check) before it replaces anything.  An entry is refused, RTGPU_ERR_INVALID_ARGUMENT,
 *              if an interpreted word is not finite (the xyz of all eight quads, aperture, focalDistance), if its stored ray is degenerate by the rule above,
 *              or if, with lens = 1, its focalDistance is not > 0.  The uninterpreted w lanes are never tested.  A refused table leaves the previous
 *              source -- plain, lens, or the camera -- exactly as it was.  RtLensSourceParams::lens above 1 or bokehShape above 2, a NULL argument, count !=
 *              width * height: RTGPU_ERR_INVALID_ARGUMENT; before rtgpu_resize: RTGPU_ERR_NOT_READY.
 *   _device    as rtgpu_set_ray_source_device: device memory of the context's device, 4-byte aligned, whose allocation holds 128 * count bytes from the
 *              pointer on; ordered behind `stream`; a multi-device context: RTGPU_ERR_UNSUPPORTED (the host entry replicates the table to every device).
 *   keeps / drops   as the ray source: only rtgpu_resize drops it.  rtgpu_get_ray_source counts the entries of a source of either kind;
 *              rtgpu_get_ray_source_kind: 0 the camera, 1 a ray source, 2 a lens source.
 * rtgpu_read_lens_source_rays[_async] write, for every pixel, the final origin and direction a pass with `params` would start from under the lens source
 * that is set -- the jitter by params->sampleOffset, the lens draws of params' sampler and the guard included -- in RtPrimaryRay's layout, words 3 and 7 zero.
 * Not a pass: nothing is walked, film, counters and queued passes are untouched.  It is what makes the definition above checkable on its own.  No lens
 * source set: RTGPU_ERR_NOT_READY; so is a source with lens = 1 under params->useBlueNoise before rtgpu_upload_scene (the draws take the scene's blue noise).
 * rtgpu_read_camera_footprints[_async] export a camera as a lens table: origin and pinhole direction as Camera::GenerateRay
 * computes them at params->sampleOffset, dDirection/dsx = r[0] * (2 / width * aspectRatio * tanHalfFoV), dDirection/dsy = r[1] * (2 / height * tanHalfFoV)
 * (r: the rows of localToWorld; film rows run bottom-up, so d/dsy has the camera's sign), dOrigin = 0, aperture and focalDistance the camera's, lensU = r[0],
 * lensV = r[1], every uninterpreted w zero.  A camera with dofEnable is accepted -- set the table with lens = 1 and its bokehShape and a pass at the
 * export's offset renders that camera's frame bit for bit; barrelDistortionVariableFactor != 0: RTGPU_ERR_UNSUPPORTED.  The _async entries take device memory
 * (16-byte aligned, held to the pointer checks above) on `stream` (NULL: the context's own) and return without synchronising.
 * --------------------------------------------------------------------------------------------- */
typedef struct RtLensRay
{
    float origin[3];     float aperture;
    float direction[3];  float focalDistance;
    float dOriginDsx[3];    float _pad2;
    float dOriginDsy[3];    float _pad3;
    float dDirectionDsx[3]; float _pad4;
    float dDirectionDsy[3]; float _pad5;
    float lensU[3];      float _pad6;
    float lensV[3];      float _pad7;
} RtLensRay;   /* 128 bytes */
typedef struct RtLensSourceParams { uint32_t lens; uint32_t bokehShape; } RtLensSourceParams;   /* lens: 0 / 1; bokehShape: 0 circle, 1 hexagon, 2 square */
int rtgpu_set_lens_source(RtgpuContext* ctx, const RtLensRay* rays, uint64_t count, const RtLensSourceParams* params);                        /* host pointer */
int rtgpu_set_lens_source_device(RtgpuContext* ctx, const RtLensRay* rays, uint64_t count, const RtLensSourceParams* params, void* stream);   /* device pointer */
int rtgpu_get_ray_source_kind(RtgpuContext* ctx, uint32_t* outKind);                                                                          /* 0 camera, 1 ray source, 2 lens source */
int rtgpu_read_lens_source_rays(RtgpuContext* ctx, const RtPassParams* params, RtPrimaryRay* out);                       /* host; synchronous */
int rtgpu_read_lens_source_rays_async(RtgpuContext* ctx, const RtPassParams* params, RtPrimaryRay* out, void* stream);   /* device */
int rtgpu_read_camera_footprints(RtgpuContext* ctx, const RtPassParams* params, RtLensRay* out);                         /* host; synchronous */
int rtgpu_read_camera_footprints_async(RtgpuContext* ctx, const RtPassParams* params, RtLensRay* out, void* stream);     /* device */

/* ---------------------------------------------------------------------------------------------
 * Denoise: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a rendered frame, guided by the first-hit planes
 * rtgpu_render_aovs writes.  It is this library's own filter, defined here operation by operation; tests/denoise_ref.py is the same text in
 * NumPy float32 and the device is held to it bit for bit.
 *   inputs     a W x H frame, rows as the sum buffer's: color H x W x 3 f32 interleaved (the sum buffer's layout); depth 1 x H x W; normal,
 *              position, albedo 3 x H x W each, channel-major (the DEPTH, NORMAL, POSITION and BASE_COLOR planes).  A pixel is valid iff its
 *              depth is finite (a miss has +inf).
 *   arithmetic f32; every a * b + c is a rounded multiply, then a rounded add; sums associate left to right as written.
 *   constants  invN = 1 / (sigmaNormal * sigmaNormal), invP = 1 / (sigmaPlane * sigmaPlane), invC[0] = 1 / (sigmaColor * sigmaColor),
 *              invC[s + 1] = invC[s] * 4 (the colour sigma halves per level).
 *   prepare    c = color * colorScale per channel; with RT_DENOISE_DEMODULATE, per channel k, d_k = albedo_k > 1e-3f ? albedo_k : 1.0f and
 *              c_k = c_k / d_k; without it d = 1 and albedo may be NULL.
 *   level s    (s = 0 .. iterations - 1, step = 1 << s; the levels ping-pong between two buffers) an invalid pixel p copies its colour.  A valid
 *              one: acc = 0, wsum = 0; for j = -2 .. 2 (rows, outermost), i = -2 .. 2 (columns): q = p + step * (i, j), skipped when outside
 *              the frame or invalid; dn = N_p - N_q, dp = P_q - P_p, dc = c_p - c_q;
 *                  xn = (dn.x * dn.x + dn.y * dn.y) + dn.z * dn.z
 *                  t  = (N_p.x * dp.x + N_p.y * dp.y) + N_p.z * dp.z,  xp = t * t
 *                  xc = (dc.x * dc.x + dc.y * dc.y) + dc.z * dc.z
 *                  x  = (xn * invN + xp * invP) + xc * invC[s]
 *                  u  = fmaxf(0, 1 - x * 0.0625f); u = u * u, four times: (1 - x / 16)^16, exactly 0 from x = 16 on and for a NaN x
 *                  w  = (h[|i|] * h[|j|]) * u with h = {0.375, 0.25, 0.0625};  acc_k = acc_k + w * c_q,k;  wsum = wsum + w
 *              the result is acc_k / wsum, or c_p when wsum == 0.
 *   finish     out_k = result_k * d_k, H x W x 3 f32 interleaved.  Non-finite colours are the caller's business.
 *   errors     a NULL context, params or buffer (albedo only with RT_DENOISE_DEMODULATE), iterations outside 1..8, a sigma or colorScale
 *              that is not finite or <= 0, a width or height of 0: RTGPU_ERR_INVALID_ARGUMENT; more than 16 Mi pixels: RTGPU_ERR_UNSUPPORTED;
 *              rtgpu_denoise before rtgpu_upload_scene / rtgpu_resize: RTGPU_ERR_NOT_READY; what rtgpu_render_aovs refuses in guideParams
 *              gets the status it gets there.
 * rtgpu_filter_atrous is a pure image filter: it needs a context, but no scene and no rtgpu_resize.  rtgpu_denoise submits the queued passes
 * (a multi-device context gathers and answers on its first device), renders the DEPTH, NORMAL, POSITION and BASE_COLOR planes of guideParams
 * through the AOV path into device scratch and filters the context's sum buffer; colorScale is the caller's (normally 1 / numPasses).  It is
 * not a pass and leaves film, both sum buffers, counters, kernel times, the photon state and the active blocks alone.  The filter's scratch is
 * 64 bytes per pixel, the call's own, grown on use and freed with the context; the host-pointer entries and rtgpu_denoise's guide planes are
 * staged in a second buffer of at most as much.
 * --------------------------------------------------------------------------------------------- */
#define RT_DENOISE_DEMODULATE 1u
/* 32 bytes */
typedef struct RtDenoiseParams
{
    uint32_t iterations;   /* 1..8 levels */
    uint32_t flags;        /* RT_DENOISE_DEMODULATE */
    float    colorScale;
    float    sigmaColor;
    float    sigmaNormal;
    float    sigmaPlane;
    uint32_t _pad[2];
} RtDenoiseParams;
/* Host pointers; synchronous. */
int rtgpu_filter_atrous(RtgpuContext* ctx, const RtDenoiseParams* params, uint32_t width, uint32_t height, const float* color, const float* depth,
                        const float* normal, const float* position, const float* albedo, float* outRGB);
/* Device pointers (16-byte aligned; outRGB must not overlap an input) on `stream` (a hipStream_t; NULL: the context's own stream): ordered
 * after the work already queued there, returns without synchronising. */
int rtgpu_filter_atrous_async(RtgpuContext* ctx, const RtDenoiseParams* params, uint32_t width, uint32_t height, const float* color,
                              const float* depth, const float* normal, const float* position, const float* albedo, float* outRGB, void* stream);
/* outRGB: host memory, height x width x 3 floats of the context's size; synchronous. */
int rtgpu_denoise(RtgpuContext* ctx, const RtDenoiseParams* params, const RtPassParams* guideParams, float* outRGB);
/* outRGB: device memory, 16-byte aligned; the guide render and the filter are ordered on `stream` as above.  The passes rendered after the
 * call wait for its read of the sum buffer. */
int rtgpu_denoise_async(RtgpuContext* ctx, const RtDenoiseParams* params, const RtPassParams* guideParams, float* outRGB, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Variance-guided denoise: the a-trous filter above with the luminance edge-stop of SVGF (Schied et al. 2017) in place of the colour one.  The
 * film's two sums -- every pass, and every second pass -- give two estimates of a pixel, a = sum / n and b = 2 * secondary / n, and (a - b)^2 is the
 * variance of the mean (the quantity rtgpu_compute_block_errors takes the root of).  A tap's luminance distance is measured against the local
 * standard deviation, and the variance is filtered alongside the colour: a converged pixel keeps its shadow edges, a noisy one gives its fireflies
 * away.  Everything not restated here is as in rtgpu_filter_atrous: validity, invN, invP, xn, xp, h, the tap order, the f32 arithmetic with every
 * multiply and add rounded on its own, sums left to right as written.  tests/denoise_var_ref.py is the same text in NumPy float32.
 *   inputs     as above, and colorHalf: H x W x 3 f32 interleaved, the sum over half of the samples (the film's secondary buffer).
 *   constants  sL2 = sigmaLum * sigmaLum.
 *   luminance  lum(c) = ((c0 + 2 * c1) + c2) * 0.25f
 *   prepare    c_k = color_k * colorScale and b_k = colorHalf_k * (2 * colorScale), both divided by d_k under RT_DENOISE_DEMODULATE as above;
 *              e = lum(c) - lum(b), v = e * e (exact for an even number of passes); an invalid pixel gets v = 0.
 *   level s    (step = 1 << s) an invalid pixel copies c and v.  A valid pixel p:
 *              the local variance: gsum = 0, gw = 0; for j = -1 .. 1 (outermost), i = -1 .. 1: q = p + (i, j) -- NOT spread by step --, skipped when
 *                  outside the frame or invalid; k = gk[|i|] * gk[|j|] with gk = {0.5, 0.25}; gsum = gsum + k * v_q; gw = gw + k.
 *                  g = gsum / gw (the centre is always taken); denom = g * sL2 + varianceFloor.
 *              the 25 taps, spread by step, as above, with
 *                  dl = lum(c_p) - lum(c_q);  xc = (dl * dl) / denom
 *                  x  = (xn * invN + xp * invP) + xc
 *                  u and w as above;  acc_k = acc_k + w * c_q,k;  vacc = vacc + (w * w) * v_q;  wsum = wsum + w
 *              the result: c_k = acc_k / wsum, v = vacc / (wsum * wsum); both stay as they are when wsum == 0.
 *              There is no per-level schedule of sigmaLum: the variance shrinks from level to level, and that does its job.
 *   finish     out_k = c_k * d_k; outVariance = v, H x W f32 (optional: may be NULL).
 *   NaN, inf   follow from the operations: a NaN denom or xc gives the tap weight 0 through fmaxf.
 *   errors     as above, and a sigmaLum or varianceFloor that is not finite or <= 0, or a NULL colorHalf: RTGPU_ERR_INVALID_ARGUMENT.
 * The four entries mirror the four above: the same stream, alignment (outVariance too) and overlap rules (no output overlaps an input or the other
 * output).  rtgpu_denoise_var filters the context's sum and secondary buffers (a multi-device context: the gathered ones); it is not a pass either,
 * and the passes rendered after an _async call wait for its read of both buffers.  The variance travels in the fourth lane of the colour records:
 * the scratch stays at 64 bytes per pixel.
 * --------------------------------------------------------------------------------------------- */
/* 32 bytes */
typedef struct RtDenoiseVarParams
{
    uint32_t iterations;     /* 1..8 levels */
    uint32_t flags;          /* RT_DENOISE_DEMODULATE, RT_DENOISE_INPUT_PREPARED (defined below, with temporal accumulation) */
    float    colorScale;
    float    sigmaLum;       /* luminance distance in standard deviations; the wrappers' default is 4 */
    float    sigmaNormal;
    float    sigmaPlane;
    float    varianceFloor;  /* added to g * sL2: what a distance is measured against where the two halves agree; default 1e-10 */
    uint32_t _pad;
} RtDenoiseVarParams;
int rtgpu_filter_atrous_var(RtgpuContext* ctx, const RtDenoiseVarParams* params, uint32_t width, uint32_t height, const float* color,
                            const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                            float* outRGB, float* outVariance);
int rtgpu_filter_atrous_var_async(RtgpuContext* ctx, const RtDenoiseVarParams* params, uint32_t width, uint32_t height, const float* color,
                                  const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                  float* outRGB, float* outVariance, void* stream);
int rtgpu_denoise_var(RtgpuContext* ctx, const RtDenoiseVarParams* params, const RtPassParams* guideParams, float* outRGB, float* outVariance);
int rtgpu_denoise_var_async(RtgpuContext* ctx, const RtDenoiseVarParams* params, const RtPassParams* guideParams, float* outRGB,
                            float* outVariance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal accumulation: the other half of SVGF.  The scene is static between uploads and updates (objects moved by rtgpu_update_objects: the next section), so reprojection is exact geometry: the world position of a
 * pixel's first hit goes through the previous frame's worldToScreen, the previous frame's accumulated estimates are fetched bilinearly around that
 * point -- each of the four taps tested against the pixel's own surface -- and blended with this frame's.  The half-sample estimate b is accumulated
 * beside the full estimate a with the same weights: the accumulated error lum(A) - lum(B) = sum w_i e_i has E[e^2] = sum w_i^2 Var(mean_i), the
 * variance of the accumulated mean, so the variance-guided filter above takes the accumulated pair as it stands (RT_DENOISE_INPUT_PREPARED).
 * Everything not restated here is as in rtgpu_filter_atrous_var: the frame layout and row order, validity (a finite depth), d_k, the f32 arithmetic
 * with every multiply and add rounded on its own, sums left to right as written.  tests/temporal_ref.py is the same text in NumPy float32.
 *   inputs     this frame: color, colorHalf H x W x 3; depth 1 x H x W; normal, position, albedo 3 x H x W (albedo only under RT_DENOISE_DEMODULATE);
 *              objectId 1 x H x W u32, optional (the OBJECT_ID plane).
 *              the previous frame: prevA, prevB H x W x 3 and prevLength H x W f32 -- the outputs outA, outB, outLength of the previous call --,
 *              prevDepth, prevNormal, prevPosition, that frame's guide planes, and prevObjectId, optional.  The object test is skipped unless both
 *              id planes are given.  All previous pointers NULL: there is no history, and every pixel starts.
 *   outputs    outA, outB H x W x 3: the accumulated full and half-sample estimates of the mean, in history space (divided by d under
 *              RT_DENOISE_DEMODULATE and never multiplied back); outLength H x W f32; outMotion 2 x H x W f32, optional.
 *   prepare    c_k = color_k * colorScale, b_k = colorHalf_k * (2 * colorScale), both divided by d_k under RT_DENOISE_DEMODULATE.
 *   start      means outA = c, outB = b, outLength = 1, outMotion = (0, 0).  An invalid pixel starts.
 *   project    M = prevWorldToScreen (rows of four, as RtCamera holds it), P = position_p; for each lane j = 0 .. 3
 *                  t_j = P.x * M[0][j] + M[3][j];  t_j = P.y * M[1][j] + t_j;  t_j = P.z * M[2][j] + t_j
 *              start unless t_2 > 0.  u = (t_0 / t_3) * 0.5f + 0.5f, v likewise from t_1;
 *                  fx = u * (float)W - prevSampleOffset[0];  fr = v * (float)H - prevSampleOffset[1];  fy = (float)(H - 1) - fr
 *              (the generator's convention: the primary ray of pixel x goes through film coordinate (x + sampleOffset) / W, film rows run bottom-up).
 *              Start unless fx > -1 && fx < W && fy > -1 && fy < H (false for a NaN; tested before any conversion to integer).
 *              outMotion = (fx - x, fy - y).
 *   taps       x0 = floorf(fx), tx = fx - x0, likewise y0, ty.  For (a, b) in (0,0), (1,0), (0,1), (1,1): q = (x0 + a, y0 + b),
 *              k = (a ? tx : 1 - tx) * (b ? ty : 1 - ty).  A tap is taken iff q is inside the frame, prevDepth_q is finite, the ids are equal (when
 *              both id planes are given), (N_p.x * N_q.x + N_p.y * N_q.y) + N_p.z * N_q.z >= normalThreshold and, with dp = P_q - P_p,
 *              fabsf((N_p.x * dp.x + N_p.y * dp.y) + N_p.z * dp.z) <= planeTolerance * depth_p.  A taken tap adds
 *                  hA_k = hA_k + k * prevA_q,k;  hB_k likewise;  ln = ln + k * prevLength_q;  ks = ks + k
 *              start unless ks > 0.
 *   blend      hA = hA / ks, hB = hB / ks;  n = fminf(ln / ks + 1, maxHistory);  alpha = fmaxf(1 / n, alphaMin);
 *                  outA_k = hA_k + alpha * (c_k - hA_k);  outB_k likewise;  outLength = n.
 *   scope      SVGF's 3 x 3 fallback search where no tap is taken, feeding the first filtered level back into the history, and reprojecting the
 *              background by direction are not part of it: a pixel whose four taps fail starts, the history is the unfiltered pair, a miss starts.
 *              A frame needs an even number of passes, at least 2, for a - b to mean anything (as rtgpu_denoise_var).  Non-finite colours are the
 *              caller's business.
 *   errors     a NULL context, params or required buffer (albedo only with RT_DENOISE_DEMODULATE), previous pointers only partly given, exactly one
 *              id plane beside a history, a parameter outside its stated range or not finite (colorScale: finite and > 0), a width or height of 0:
 *              RTGPU_ERR_INVALID_ARGUMENT; more than 16 Mi pixels: RTGPU_ERR_UNSUPPORTED; the _async entry: a buffer that is not 16-byte aligned, an
 *              output that overlaps an input or another output: RTGPU_ERR_INVALID_ARGUMENT.
 * RT_DENOISE_INPUT_PREPARED, for rtgpu_filter_atrous_var and its three siblings: color and colorHalf are taken as c and b themselves -- no colorScale
 * multiply, no doubling, no division; the finish still multiplies by d under RT_DENOISE_DEMODULATE.  (outA, outB) go straight into the filter with it.
 *
 * rtgpu_temporal_accumulate is a pure image operation like rtgpu_filter_atrous_var, with its rules: a context, but no scene and no rtgpu_resize.
 * rtgpu_denoise_temporal keeps the history in the context.  It submits the queued passes and gathers peers as rtgpu_denoise_var does, renders the DEPTH,
 * NORMAL, POSITION, BASE_COLOR and OBJECT_ID planes of guideParams through the AOV path, accumulates the sum and secondary buffers against the stored
 * history (none: every pixel starts), stores the new history with these guides and guideParams' worldToScreen and sampleOffset, and filters (outA, outB)
 * with `filter`, its flags | RT_DENOISE_INPUT_PREPARED and its colorScale taken as 1; filter == NULL: no spatial filter, outRGB_k = outA_k * d_k and
 * outVariance is not written.  params->prevWorldToScreen and prevSampleOffset are ignored: the context remembers its own (guideParams' worldToScreen must
 * therefore be the matrix of guideParams' own localToWorld: the host mirror's Camera computes it in SetPerspective, not in SetTransform).  The result is by definition
 * the composition of the two pure entries on the same planes.  rtgpu_temporal_reset drops the history, and so do rtgpu_resize, rtgpu_set_shard and
 * rtgpu_upload_scene (rtgpu_update_objects does not: the next section); rtgpu_reset does not -- resetting the film every frame is the use case.  Like the other denoise calls these are not passes: film,
 * both sum buffers, counters, kernel times, the photon state and the active blocks stay as they are, and the passes rendered after an _async call wait
 * for its read of both sum buffers.  The history is 128 bytes per pixel (this frame's and the previous one's, four 16-byte records each: {A, length},
 * {B, id}, {N, valid}, {P, 0}), the call's own, grown on use and freed with the context; guides and the accumulated pair are staged in the filter's
 * second buffer (at most 84 bytes per pixel), and the pure entries pack the caller's history into the filter's 64-byte records.
 * --------------------------------------------------------------------------------------------- */
#define RT_DENOISE_INPUT_PREPARED 2u
/* 96 bytes */
typedef struct RtTemporalParams
{
    uint32_t flags;                /* RT_DENOISE_DEMODULATE */
    float    colorScale;           /* normally 1 / passes of this frame */
    float    alphaMin;             /* floor of the blend factor, (0, 1]; the wrappers' default is 0.1 */
    float    maxHistory;           /* cap of the history length, >= 1; default 64 */
    float    normalThreshold;      /* a tap needs N_p . N_q >= this; [-1, 1]; default 0.9 */
    float    planeTolerance;       /* a tap needs |N_p . (P_q - P_p)| <= this * depth_p; > 0; default 0.01 */
    float    prevSampleOffset[2];  /* RtPassParams::sampleOffset of the pass the previous guides were rendered with */
    float    prevWorldToScreen[16];/* RtCamera::worldToScreen of that pass */
} RtTemporalParams;
/* Host pointers; synchronous. */
int rtgpu_temporal_accumulate(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                              const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                              const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth,
                              const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB,
                              float* outLength, float* outMotion);
/* Device pointers on `stream`, as rtgpu_filter_atrous_var_async. */
int rtgpu_temporal_accumulate_async(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                    const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                    const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength,
                                    const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                    float* outA, float* outB, float* outLength, float* outMotion, void* stream);
/* outRGB (and outVariance, optional): host memory of the context's size; synchronous. */
int rtgpu_denoise_temporal(RtgpuContext* ctx, const RtTemporalParams* params, const RtDenoiseVarParams* filter /* NULL: no spatial filter */,
                           const RtPassParams* guideParams, float* outRGB, float* outVariance);
/* outRGB, outVariance: device memory, 16-byte aligned, on `stream` as rtgpu_denoise_var_async. */
int rtgpu_denoise_temporal_async(RtgpuContext* ctx, const RtTemporalParams* params, const RtDenoiseVarParams* filter, const RtPassParams* guideParams,
                                 float* outRGB, float* outVariance, void* stream);
int rtgpu_temporal_reset(RtgpuContext* ctx);

/* ---------------------------------------------------------------------------------------------
 * Temporal accumulation that follows moving objects.  Between two frames rtgpu_update_objects may have moved objects; a pixel's surface point then was
 * somewhere else in the previous frame, and perhaps under another object id (the update reorders the object table).  For every CURRENT object id o there is
 * a record RtObjectMotion: m takes a current world position to the world position the same surface point had in the previous frame (rows of four, the row
 * convention of `project` above); prevId is the id the object had in the previous frame's planes; moved == 0: the object stood still.
 * Everything not restated here is rtgpu_temporal_accumulate.
 *   per pixel  with a valid hit and id o = objectId_p < numObjects: if moved[o] == 0, P' = P_p and N' = N_p (a select: the bits of the static call); otherwise
 *              for lanes j = 0 .. 2
 *                  P'_j = P.x * m[0][j] + m[3][j];  P'_j = P.y * m[1][j] + P'_j;  P'_j = P.z * m[2][j] + P'_j
 *                  N'_j = N.x * m[0][j];            N'_j = N.y * m[1][j] + N'_j;  N'_j = N.z * m[2][j] + N'_j      (not renormalised)
 *              every multiply and add rounded on its own.  A pixel whose id is >= numObjects starts; the table is never read out of range.
 *   project    uses P'.
 *   taps       a tap is taken iff q is inside the frame, prevDepth_q is finite, prevObjectId_q == prevId[o], (N'.x * N_q.x + N'.y * N_q.y) + N'.z * N_q.z >=
 *              normalThreshold and, with dp = P_q - P', fabsf((N'.x * dp.x + N'.y * dp.y) + N'.z * dp.z) <= planeTolerance * depth_p.
 *   the rest   outMotion, blend and start rules are unchanged; what the caller keeps as the next history are the CURRENT N, P and ids.
 *   scope      rigid motions.  Under a scale N' is no unit normal and the plane distance is measured in the previous frame's units: the two surface tests
 *              are then approximate, but defined.  Lighting that changed because a light or an occluder moved is not reprojected: the history lags behind
 *              it by what alphaMin allows.
 *   errors     as rtgpu_temporal_accumulate, and: objects NULL or numObjects == 0, objectId NULL, prevObjectId NULL beside a history:
 *              RTGPU_ERR_INVALID_ARGUMENT; the _async entry: a table that is not 16-byte aligned device memory.
 * The table is host memory for the synchronous entry and device memory for the _async one.
 *
 * rtgpu_denoise_temporal builds the table itself.  With the history it keeps, per current object, the id and the transform the object had when the history was
 * stored; rtgpu_update_objects carries them through its previousIndex (through several updates, if there are several between two frames) and no longer
 * drops the history.  At the next call moved[o] = 0 when the 16 words of the transform are bit-equal to the stored ones; otherwise
 * m = invTransform_now * transform_then (row convention: world now -> local -> world then), every element computed in double, the four products of a dot
 * product summed left to right, and rounded to float once.  A product of two floats is exact in double, so neither a contraction into fused multiply-adds
 * nor NumPy's float64 arithmetic can round the sum differently: tests/temporal_moving_ref.py builds the same table.  When no update happened since the
 * history was stored the call launches what it launched before objects could move, with the same arguments.
 * --------------------------------------------------------------------------------------------- */
/* 80 bytes (five 16-byte loads) */
typedef struct RtObjectMotion { float m[16]; uint32_t prevId; uint32_t moved; uint32_t _pad[2]; } RtObjectMotion;
int rtgpu_temporal_accumulate_moving(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                     const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                     const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth,
                                     const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB,
                                     float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects);
int rtgpu_temporal_accumulate_moving_async(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                           const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                           const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength,
                                           const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                           float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects,
                                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Clipping the history.  Reprojection follows a pixel's surface, not the light on it: when a shadow arrives, the history carries the sunlight on at what alphaMin
 * allows.  The remedy of the image-space kind (TAA, ReLAX, ReBLUR): the reprojected history is clipped to the mean +- gamma standard deviations of THIS frame's
 * colours over the pixel's own surface in a small window, and the further it had to be pulled, the shorter its history length becomes.  Where nothing clips the
 * result is the bits of the call without.  Everything not restated here is rtgpu_temporal_accumulate_moving, and with objects == NULL and numObjects == 0
 * rtgpu_temporal_accumulate; the rules of every operation are theirs: f32, every multiply and add rounded on its own, sums in the order written, correctly
 * rounded / and sqrtf.  tests/temporal_clip_ref.py is the same text in NumPy float32.
 *   moments    for a valid pixel p, over the window pixels q = (x + dx, y + dy), dy = -r .. r outer, dx = -r .. r inner, p itself included.  q counts iff it is
 *              inside the frame, depth_q is finite, objectId_q == objectId_p (when the objectId plane is given),
 *              (N_p.x * N_q.x + N_p.y * N_q.y) + N_p.z * N_q.z >= normalThreshold and, with dp = P_q - P_p,
 *              fabsf((N_p.x * dp.x + N_p.y * dp.y) + N_p.z * dp.z) <= planeTolerance * depth_p -- this frame's guides and the pixel's own N and P, never the
 *              moved pair.  Each counted q adds   cnt = cnt + 1;  s1_k = s1_k + c_q,k;  s2_k = s2_k + c_q,k * c_q,k   (c: the prepared colour, in history
 *              space).  Then   mu_k = s1_k / cnt;  var_k = fmaxf(s2_k / cnt - mu_k * mu_k, 0);  g_k = gamma * sqrtf(var_k).
 *   clip       where the pixel blends (ks > 0) and cnt >= minCount, behind hA = hA / ks, hB = hB / ks:
 *                  lo_k = mu_k - g_k;  hi_k = mu_k + g_k;  hA'_k = fminf(fmaxf(hA_k, lo_k), hi_k);  hB'_k = hB_k + (hA'_k - hA_k)
 *              B is shifted, not clipped: clipped into the same box A - B would be zero, and the variance-guided filter would take the pixel for converged
 *              exactly where its history was just thrown away.  The shift keeps the accumulated variance estimate.
 *   anti-lag   e = (fabsf(hA'_0 - hA_0) + fabsf(hA'_1 - hA_1)) + fabsf(hA'_2 - hA_2);  wd = (g_0 + g_1) + g_2;  f = e > 0 ? wd / (wd + e) : 1;
 *                  n = fminf((ln / ks) * f + 1, maxHistory)
 *              alpha and the blend as before, over hA' and hB'.  With e = 0 the factor is exactly 1 and (ln / ks) * 1 is ln / ks: a pixel that does not clip
 *              carries the bits of the call without a clip.  A pixel with cnt < minCount, a pixel that starts and an invalid pixel are untouched, with f = 1.
 *   outputs    those of the call without, and outConfidence, H x W f32, optional: f.
 *   scope      the statistics are this frame's: a window that straddles a shadow edge is wide and lets a band of r pixels lag on; under heavy-tailed noise the
 *              sample deviation underestimates, and a small gamma darkens a static image.  Neither is repaired ("History clipping", has their
 *              size).  Non-finite colours remain the caller's business.
 *   errors     as rtgpu_temporal_accumulate_moving -- but objects may be NULL with numObjects == 0: then no object moved --, and: clip NULL on the pure entries,
 *              radius outside 1 .. 3, minCount outside 1 .. 49, gamma not finite or outside [0, 1e6]: RTGPU_ERR_INVALID_ARGUMENT; the _async entry holds
 *              outConfidence to the alignment and overlap rules of the other outputs.
 * rtgpu_denoise_temporal_clip is rtgpu_denoise_temporal with the clip: by definition the composition of the pure entries, the motion table built after an update
 * as that call builds it.  clip == NULL: rtgpu_denoise_temporal itself, word for word and launch for launch (outConfidence is then not written).  outConfidence:
 * memory of outRGB's kind.  The moments are 32 bytes per pixel of scratch of the clipped calls' own, grown on use and freed with the context.
 * --------------------------------------------------------------------------------------------- */
typedef struct RtTemporalClip {   /* 16 bytes */
    uint32_t radius;     /* window (2r+1)^2 around the pixel in THIS frame; 1, 2 or 3 */
    float    gamma;      /* half-width of the box in standard deviations; finite, [0, 1e6] */
    uint32_t minCount;   /* clip only where at least this many window pixels lie on the pixel's surface; 1 .. 49 */
    uint32_t _pad;
} RtTemporalClip;
int rtgpu_temporal_accumulate_clip(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                   const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                   const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth,
                                   const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB,
                                   float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects, const RtTemporalClip* clip,
                                   float* outConfidence);
int rtgpu_temporal_accumulate_clip_async(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                         const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                         const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength,
                                         const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                         float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects,
                                         const RtTemporalClip* clip, float* outConfidence, void* stream);
int rtgpu_denoise_temporal_clip(RtgpuContext* ctx, const RtTemporalParams* params, const RtDenoiseVarParams* filter, const RtPassParams* guideParams,
                                float* outRGB, float* outVariance, const RtTemporalClip* clip, float* outConfidence);
int rtgpu_denoise_temporal_clip_async(RtgpuContext* ctx, const RtTemporalParams* params, const RtDenoiseVarParams* filter, const RtPassParams* guideParams,
                                      float* outRGB, float* outVariance, const RtTemporalClip* clip, float* outConfidence, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal accumulation over chain guides: reflections in the history.  With first-hit guides every pixel inside a mirror reprojects the mirror's own plane,
 * which stands still while the reflected image slides under a moving camera; the surface tests pass (the same mirror, normal and id), and the history blends
 * last frame's reflection into this frame's at the wrong place.  The remedy is the one ReBLUR and ReLAX use for specular motion: reproject the virtual image
 * (RT_AOV_VIRTUAL_POSITION above), test the taps on the chain guides -- the reflected surface stands still in world space -- and keep histories of different
 * chain lengths apart.  Everything not restated here is rtgpu_temporal_accumulate_clip; tests/temporal_chain_ref.py is the same text in NumPy float32.
 *   inputs     normal, position, depth, albedo and objectId are chain guides, at the guide vertex (rtgpu_render_aovs_chain).  RtTemporalChain adds this frame's
 *              virtualPosition 3 x H x W f32 (V), chainLength 1 x H x W u32 (k), chainDistance 1 x H x W f32 (D), and the previous frame's prevChainLength
 *              1 x H x W u32, required exactly when a history is given.  Chain lengths are at most RT_AOV_CHAIN_MAX, as the chain call writes them; the planes are
 *              not range-checked, and a length of 0xFFFFFFFF is undefined here (in the moments it reads as an invalid pixel).  clip may be NULL: no clipping, outConfidence is not written.  objects may be NULL
 *              with numObjects == 0.
 *   project    uses V_p in P_p's place; outMotion is therefore the virtual motion.
 *   tolerance  planeTolerance * chainDistance_p replaces planeTolerance * depth_p, in the taps and in the moments: inside a reflection the last segment's
 *              length is the wrong scale.  For k == 0 the two are the same word.
 *   taps       a tap is taken iff the conditions of the call without hold -- over N_p, P_p and the ids of the guide planes -- and prevChainLength_q ==
 *              chainLength_p: a surface seen directly and the same surface seen in a tinted mirror do not share a colour history.
 *   moments    a window pixel counts iff the conditions of the call without hold (validity: chainDistance_q finite, which is depth_q finite) and
 *              chainLength_q == chainLength_p.
 *   moving     when objects != NULL a pixel with chainLength_p > 0 starts; a pixel with chainLength_p == 0 follows the moving rules unchanged: it projects
 *              P' (made from P_p, not from V_p) and tests its taps against P' and N'.
 *   the rest   validity, prepare, blend, clip, anti-lag and the outputs are unchanged.  What the caller keeps as the next history are the current guides and
 *              chainLength.
 *   identity   with chainLength and prevChainLength all zero, virtualPosition the words of position and chainDistance the words of depth, every output is the
 *              words of rtgpu_temporal_accumulate_clip; with clip == NULL, of rtgpu_temporal_accumulate[_moving].
 *   scope      plane mirrors, any number of them: exact.  Curved mirrors and refraction: V is an approximation, fenced by the tap tests -- where it fails the
 *              pixel starts.  The virtual image of a scene in which something moved, possibly the mirror, is not followed: dropping the history there costs
 *              noise, keeping it would ghost.  On glass a pass's guides pick reflect or refract per pixel by the pass's own draw, so per-pixel chain lengths
 *              differ from frame to frame and most glass pixels start.
 *   errors     those of rtgpu_temporal_accumulate_clip, except that clip == NULL is allowed; and RTGPU_ERR_INVALID_ARGUMENT for: chain NULL; any of its three
 *              current planes NULL; prevChainLength given without a history, or missing beside one; the _async entry: any of these planes violating the
 *              alignment or overlap rules.
 * rtgpu_denoise_temporal_chain is by definition rtgpu_render_aovs_virtual -- the DEPTH, NORMAL, POSITION, BASE_COLOR, OBJECT_ID, CHAIN_LENGTH, CHAIN_DISTANCE
 * and VIRTUAL_POSITION planes of guideParams under `chain` -- followed by the pure entry on the same planes and then the filter: the composition
 * rtgpu_denoise_temporal_clip is, over chain planes.  It takes its chain from its argument: rtgpu_set_guide_chain does not affect it (and the entries without
 * keep answering RTGPU_ERR_UNSUPPORTED while one is set).  With chain->maxChain == 0 its outputs are the words of rtgpu_denoise_temporal_clip.  The motion
 * table is built as that call builds it and passed only when an update happened since the history was stored; pixels with k > 0 then start for that frame.
 * The chain length travels in the free lane of the {P, .} history record -- the entries without write 0.0f there, which is k = 0 bit for bit -- so the
 * history stays 128 bytes per pixel, and a history the entries without wrote is valid input here.  The other way round it is not: the context remembers that
 * the stored history was written by this entry, and rtgpu_denoise_temporal[_clip][_async] then treat it as no history (every pixel starts) and overwrite it.
 * Multi-device, shard, active-block, stream and "not a pass" rules are those of rtgpu_denoise_temporal_clip.
 * Measured (one MI355X, one run; Sponza-class 1920 x 1080 with a mirror and a glass sphere, maxChain 3, 2 passes a frame, 16 frames of 0.25 degrees of yaw;
 * tools/bench_temporal.py --chain 3 --mirror --clip): the mirror's pixels keep a mean history length of 15.6 (1 % start in the last frame), the
 * glass sphere's 8.3 (20 % start).  The pure entry (timed as a call: pack and kernels) takes 0.158 ms against 0.148 for the entry without on the same planes (clipped 0.315 against
 * 0.302), the whole call 2.65 ms against rtgpu_denoise_temporal's 1.48 (1.69 against 1.32 where nothing is specular): the guide render through the chain call.  By relative MSE the
 * call does NOT beat the call with first-hit guides: inside the mirror 0.097 against 0.048 filtered (clipped 0.052 against 0.040; at 1 degree a frame 0.069 against
 * 0.053), on the glass sphere 1.09 against 0.10.  The variance-guided filter over chain guides loses what the history gains (unfiltered and unclipped the mirror
 * reads 0.19 against 0.43), and at two passes a frame the measure does not see the ghost the first-hit history drags along.
 * --------------------------------------------------------------------------------------------- */
typedef struct RtTemporalChain {   /* 32 bytes */
    const float*    virtualPosition;   /* 3 x H x W: RT_AOV_VIRTUAL_POSITION */
    const uint32_t* chainLength;       /* 1 x H x W: RT_AOV_CHAIN_LENGTH */
    const float*    chainDistance;     /* 1 x H x W: RT_AOV_CHAIN_DISTANCE */
    const uint32_t* prevChainLength;   /* 1 x H x W: the previous frame's chainLength; NULL exactly when there is no history */
} RtTemporalChain;
int rtgpu_temporal_accumulate_chain(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                    const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                    const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth,
                                    const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB,
                                    float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects,
                                    const RtTemporalClip* clip /* NULL: none */, float* outConfidence, const RtTemporalChain* chain);
int rtgpu_temporal_accumulate_chain_async(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                          const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                          const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength,
                                          const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                          float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects,
                                          uint32_t numObjects, const RtTemporalClip* clip, float* outConfidence, const RtTemporalChain* chain, void* stream);
int rtgpu_denoise_temporal_chain(RtgpuContext* ctx, const RtTemporalParams* params, const RtDenoiseVarParams* filter, const RtPassParams* guideParams,
                                 const RtAovChain* chain, float* outRGB, float* outVariance, const RtTemporalClip* clip /* NULL: none */,
                                 float* outConfidence);
int rtgpu_denoise_temporal_chain_async(RtgpuContext* ctx, const RtTemporalParams* params, const RtDenoiseVarParams* filter,
                                       const RtPassParams* guideParams, const RtAovChain* chain, float* outRGB, float* outVariance,
                                       const RtTemporalClip* clip, float* outConfidence, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal accumulation that follows deforming meshes.  rtgpu_update_mesh moves a mesh's vertices; a pixel's surface point then was somewhere else in the
 * previous frame, and no matrix says where.  The pixel itself does: the AOV call gives the triangle its first hit lies on (RT_AOV_SUB_OBJECT_ID, relative to
 * the mesh, in the order of the mesh's triangle records) and the hit's barycentrics (RT_AOV_BARYCENTRICS), and v0 + u edge1 + v edge2 of the record that
 * triangle had a frame ago is where the same surface point was, in the mesh's local space.  A record of the motion table with moved == RT_MOTION_DEFORMED
 * marks an object whose mesh was deformed: its m takes the mesh-LOCAL position the point had then to the world position it had then (the object's transform
 * of that time, word for word), _pad[0] is the first record of its mesh in prevTriangles and _pad[1] its triangle count; prevId is as before.  Records with
 * moved 0 or 1 follow the rules of rtgpu_temporal_accumulate_moving, bit for bit.  Everything not restated here is rtgpu_temporal_accumulate_moving and
 * rtgpu_temporal_accumulate_clip (clip may be NULL: no clipping, outConfidence is not written); tests/temporal_deform_ref.py is the same text in NumPy float32.
 *   per pixel  with a valid hit, o = objectId_p < numObjects and moved[o] == RT_MOTION_DEFORMED: t = subObjectId_p, (u, v) = barycentrics_p.  The pixel starts
 *              unless t < _pad[1] and _pad[0] + t < numPrevTriangles, the sum taken without 32-bit wrap-around: neither the table nor the triangle array is ever
 *              read out of range, whatever the planes or a device-resident table hold.  Otherwise, with T = prevTriangles[_pad[0] + t], for lanes k = 0 .. 2
 *                  L_k = T.edge1_k * u + T.v0_k;  L_k = T.edge2_k * v + L_k
 *              and for lanes j = 0 .. 2
 *                  P'_j = L.x * m[0][j] + m[3][j];  P'_j = L.y * m[1][j] + P'_j;  P'_j = L.z * m[2][j] + P'_j
 *              every multiply and add rounded on its own.  N' = N_p: the shading normal is not carried back.
 *   project, taps, blend, clip, outputs   unchanged: P' is projected, a tap is taken iff prevObjectId_q == prevId[o] and it passes the two surface tests against
 *              P' and N'; what the caller keeps as the next history are the CURRENT N, P and ids.  The moments of a clip never use the moved pair.
 *   identity   with no record of moved == RT_MOTION_DEFORMED every output is the words of rtgpu_temporal_accumulate_clip; with clip == NULL, of
 *              rtgpu_temporal_accumulate_moving.
 *   scope      deformations that keep the topology.  The turn the deformation gives the normal is left to normalThreshold, and so is a rigid move of the same
 *              object between the same two frames: its position is followed exactly (m is the transform of then), its normal is not turned back.  Lighting that
 *              changed with the shape is not reprojected (clip it).  Not followed inside reflections: the _chain entries have no such variant.
 *   errors     those of rtgpu_temporal_accumulate_clip, except that clip == NULL is allowed; and RTGPU_ERR_INVALID_ARGUMENT for: deform NULL or objects NULL;
 *              either plane NULL; prevTriangles NULL with numPrevTriangles > 0; _pad != 0; the host entry: a record with moved > RT_MOTION_DEFORMED, or a
 *              deformed record with _pad[0] + _pad[1] > numPrevTriangles; the _async entry (which cannot read a device table: there the kernel's range test
 *              alone stands): either plane violating the alignment or overlap rules, prevTriangles not 4-byte aligned.
 * The table, the planes and prevTriangles are host memory for the synchronous entry and device memory for the _async one (deform itself is host memory).
 *
 * rtgpu_set_deform_tracking(ctx, 1) lets rtgpu_denoise_temporal[_clip][_async] follow rtgpu_update_mesh; off (the default) nothing changes, no launch and no
 * byte.  With it on, an accepted rtgpu_update_mesh of a mesh that has not been updated since the history was stored copies the mesh's triangle records, device
 * to device on the update's stream and before its first kernel, into a snapshot array over the scene's triangle numbering (36 bytes per triangle of the scene,
 * allocated with the first snapshot, freed with the scene); further updates of that mesh before the next temporal call leave the snapshot alone -- it shows
 * the mesh as the history saw it.  The mesh's objects keep the id they had and are marked deformed.  The next rtgpu_denoise_temporal[_clip][_async] then
 * renders SUB_OBJECT_ID and BARYCENTRICS beside its five guide planes and is by definition the pure entry above on those planes, the snapshot (numPrevTriangles
 * = the scene's triangle count) and the table of rtgpu_denoise_temporal with, for every marked object, moved = RT_MOTION_DEFORMED, m = the words of the
 * transform the object had when the history was stored, _pad = { RtMesh::firstTriangle, RtMesh::numTriangles } and prevId as rtgpu_update_objects carried it.
 * Storing a history invalidates every snapshot; rtgpu_upload_scene drops them with the history; a refused update takes none.  A mesh updated while tracking
 * was off, or before a history existed, has no snapshot: its objects get prevId = 0xFFFFFFFF as ever.  Without a marked object the calls launch what they
 * launched before, with the same arguments.  rtgpu_denoise_temporal_chain ignores tracking: there a deformed mesh's pixels start.  A multi-device context sets
 * every peer (never run on two devices so far).
 * --------------------------------------------------------------------------------------------- */
#define RT_MOTION_DEFORMED 2u      /* RtObjectMotion::moved */
typedef struct RtTemporalDeform {  /* 32 bytes */
    const uint32_t*   subObjectId;    /* 1 x H x W: this frame's RT_AOV_SUB_OBJECT_ID */
    const float*      barycentrics;   /* 2 x H x W: this frame's RT_AOV_BARYCENTRICS  */
    const RtTriangle* prevTriangles;  /* [numPrevTriangles]: the records as they were when the history was stored */
    uint32_t numPrevTriangles, _pad;
} RtTemporalDeform;
int rtgpu_temporal_accumulate_deform(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                     const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                     const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth,
                                     const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB,
                                     float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects,
                                     const RtTemporalClip* clip /* NULL: none */, float* outConfidence, const RtTemporalDeform* deform);
int rtgpu_temporal_accumulate_deform_async(RtgpuContext* ctx, const RtTemporalParams* params, uint32_t width, uint32_t height, const float* color,
                                           const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo,
                                           const uint32_t* objectId, const float* prevA, const float* prevB, const float* prevLength,
                                           const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                           float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects,
                                           uint32_t numObjects, const RtTemporalClip* clip, float* outConfidence, const RtTemporalDeform* deform, void* stream);
int rtgpu_set_deform_tracking(RtgpuContext* ctx, int enable);

/* rtgpu_postprocess over a caller's image (host memory, height x width x 3 floats of the context's size) in place of the sum buffer -- a
 * denoised frame, say: the same kernels, the same restrictions, and the same bits for the same input. */
int rtgpu_postprocess_from(RtgpuContext* ctx, const RtPostprocessParams* params, const float* rgbHost, uint32_t* frontBufferBGRA);

/* Known-answer-test hooks.  They evaluate the DEVICE implementation of one hot-path function (the code the traversal and shading
 * kernels call, rt_device_*.h) on caller-provided records, so that tests can hold the HIP functions directly against vectors produced
 * by the reference's own translation units (tests/golden/) without going through any CPU
 * restatement.  Host pointers, synchronous, not performance relevant.
 *   rtgpu_kat         func = function id of the .kat fixture header (tests/golden/README.md: Sin/SinCos/FastLog/FastACos/FastATan2,
 *                     SamplingHelpers, BuildOrthonormalBasis, Fresnel*, Refract3/Reflect3, Ray::Ray, TransformRay_Unsafe,
 *                     FastInverseNoScale, Intersect_BoxRay(_TwoSided), Intersect_TriangleRay, shape Intersect/Sample/Pdf/
 *                     EvaluateIntersection, ILight::Illuminate/GetRadiance/Emit, BSDF::Sample/Evaluate/Pdf, Camera::GenerateRay/
 *                     WorldToFilm/PdfW, Film splat pixel, Packed* photons, DebugRenderer triangle colour); in: n records of inStride
 *                     floats (integers bit-cast), out: n records of outStride floats.
 *   rtgpu_kat_sampler GenericSampler::ResetPixel + GetInt/GetFloat (Core/Sampling/GenericSampler.cpp:69-113): record =
 *                     {x, y, useBlueNoise, numDims, seed[numDims]}; count draws per record.  blueNoise: 128*128*4 uint16 or NULL.
 *   rtgpu_kat_mesh    MeshShape::Traverse / Traverse_Shadow / EvaluateIntersection (Core/Shapes/MeshShape.cpp:134-328) through the
 *                     traversal state machine of the path tracer, on the uploaded scene's single mesh object: rays = n * {origin[3],
 *                     direction[3], tmax}, out = n * 19 words {objectId (7 on a hit), triangle, distance, u, v, anyHit, tangent[4],
 *                     normal[4], texCoord[4], material}.
 *   rtgpu_kat_postprocess  the per-pixel body of Viewport::PostProcessTile (the function rtgpu_postprocess's kernels call) on n records, each with
 *                     its own params, at pixel (0, 0), without bloom: rgb = n * 3 sum-buffer floats, outBGR = n words 0x00RRGGBB,
 *                     outToneMapped (n * 3, may be NULL) = the floats Vector4::ToBGR quantises, dithering included.  colorScale is computed
 *                     on the host as rtgpu_postprocess does.  An unknown tone mapper or numPasses = 0 in any record: INVALID_ARGUMENT.
 *   rtgpu_kat_blur    Bitmap::GaussianBlur(sigma, 8) in place on a tight float3 image in host memory: the window plan and the two kernel
 *                     launches of rtgpu_postprocess's bloom levels.  Needs no rtgpu_resize.  Refused as there (RTGPU_ERR_UNSUPPORTED, the
 *                     image untouched) unless width is a multiple of 4 and both sizes are <= 4096 and > 2 * wu + 1 for this sigma's window. */
int rtgpu_kat(RtgpuContext* ctx, uint32_t func, const float* in, uint32_t inStride, float* out, uint32_t outStride, uint32_t n);
int rtgpu_kat_sampler(RtgpuContext* ctx, const uint16_t* blueNoise, const uint32_t* in, uint32_t inStride, uint32_t count, uint32_t n,
                      uint32_t* outInts, float* outFloats);
int rtgpu_kat_mesh(RtgpuContext* ctx, const float* rays, uint32_t n, uint32_t* out);
int rtgpu_kat_postprocess(RtgpuContext* ctx, const RtPostprocessParams* params, const float* rgb, uint32_t n, uint32_t* outBGR, float* outToneMapped);
int rtgpu_kat_blur(RtgpuContext* ctx, float* rgbHost, uint32_t width, uint32_t height, float sigma);

/* --- measurement hooks (bench.py) ---------------------------------------------------------------
 * Per-kernel-class GPU time in milliseconds accumulated since rtgpu_reset, measured with HIP events
 * on the stream each kernel is launched on when timing is enabled (with more than one batch lane the kernels of
 * different batches overlap, so the classes' times can add up to more than the wall time).  names[i] are static
 * strings. */
#define RTGPU_NUM_KERNEL_CLASSES 8
int rtgpu_enable_timing(RtgpuContext* ctx, int enable);
int rtgpu_get_kernel_times(RtgpuContext* ctx, double ms[RTGPU_NUM_KERNEL_CLASSES],
                           uint64_t launches[RTGPU_NUM_KERNEL_CLASSES],
                           const char* names[RTGPU_NUM_KERNEL_CLASSES]);

/* Which traversal kernel serves the uploaded scene with the intersection counters off, and the bytes its walk fetches from: the node
 * records, the leaves' exact boxes and the triangles (what decides where the memory system serves the walk's divergent fetches from;
 * bench.py prices the kernel's access rate against the microbenchmark's figure for this footprint).  Diagnostic, like the timing calls. */
#define RTGPU_WALK_BINARY 0u   /* k_trace: the reference's binary tree (also every scene with the counters on) */
#define RTGPU_WALK_WIDE   1u   /* k_trace_wide: 4-wide collapse of a single mesh's tree */
#define RTGPU_WALK_WIDE2  2u   /* k_trace_wide2: 4-wide top level over 4-wide mesh trees */
typedef struct RtWalkInfo
{
    uint32_t kernel, reserved;
    uint64_t nodeBytes, leafBoxBytes, triangleBytes;
} RtWalkInfo;
int rtgpu_get_walk_info(RtgpuContext* ctx, RtWalkInfo* out);

/* Beam lists: while a frame accumulates under a still pinhole camera, the camera rays of a dense batch over a single-mesh scene take their leaves from
 * per-tile lists (a tile = 64 consecutive slots of the slot table = one 8 x 8 pixel block) built once, with the second batch the camera serves, in place of
 * walking the tree on every pass.  Results do not depend on it, bit for bit.  RTGPU_BEAM_LISTS=0 turns it off.
 *   rtgpu_set_beam_margin    m, in pixels: a pass whose |sampleOffset| exceeds m on an axis walks the tree.  The lists hold every leaf a ray of the tile can
 *                            pass at offsets within m, so a larger m serves more passes from longer lists.  Default 1.5 (3 x the default
 *                            antiAliasingSpread: sampleOffset is normal with that deviation); a renderer with another spread sets 3 x its own.
 *   rtgpu_get_beam_list_info synchronises, then reports (of the first device of a multi-device context):
 *       builds               build launches since the context was created (a camera that changes with every batch never causes one)
 *       allocations          builds that took new device arrays (numTiles x capacity x 8 bytes and numTiles x 4): a build behind idle lanes rewrites the
 *                            arrays the context has, so a caller who synchronises between rebuilds allocates once
 *       retiredArrays        arrays of earlier builds that launches in flight could still read when the call was made (before it synchronised, which
 *                            frees them, as every synchronising call does); never more than 4
 *       valid                lists exist for the last batch's camera; capacity, numTiles, margin: theirs
 *       packetsScanned / packetsWalkedOffset / packetsWalkedNoList   packets (waves of 64 camera rays) of launches that had lists: served from their
 *                            tile's list, walked because their pass's offset exceeds the margin, walked because their tile has no list (more leaves than
 *                            the capacity) or the packet straddles two tiles (a slot table whose length is no multiple of 64)
 *   rtgpu_read_beam_lists    the lists themselves: counts[numTiles] (0xFFFFFFFF: no list) and entries[numTiles * capacity] as {leaf reference, bits of dmin}
 *                            pairs, ascending; fromHost != 0: not the device's arrays but what the pure host builder makes of the same tree, slot table and
 *                            key (the reference the build kernel is tested against).  RTGPU_ERR_NOT_READY without valid lists. */
typedef struct RtBeamListInfo
{
    uint64_t builds, packetsScanned, packetsWalkedOffset, packetsWalkedNoList;
    uint32_t valid, capacity, numTiles;
    float    margin;
    uint64_t allocations;
    uint32_t retiredArrays, reserved;
} RtBeamListInfo;
int rtgpu_set_beam_margin(RtgpuContext* ctx, float pixels);
int rtgpu_get_beam_list_info(RtgpuContext* ctx, RtBeamListInfo* out);
int rtgpu_read_beam_lists(RtgpuContext* ctx, int fromHost, uint32_t* counts, uint32_t* entries);

/* How a multi-device context (rtgpu_create_multi) exchanges the peers' tiles at read-back, and why -- so that a first run on a real multi-GPU node
 * explains itself (the reference has no counterpart: its only fan-out is Core/Utils/ThreadPool.cpp:57-117 under Viewport.cpp:244-262).
 *   gatherMode    0 one device (nothing to gather), 1 a kernel on the first device reads the peers' sum buffers in place (peer access over xGMI),
 *                 2 hipMemcpyPeerAsync into staging buffers of the first device, then the same kernel
 *   gatherReason  why mode 2: 0 not staged, 1 RTGPU_MULTI_STAGED=1, 2 hipDeviceCanAccessPeer said no for `reasonDevice`,
 *                 3 hipDeviceEnablePeerAccess failed for `reasonDevice` (reasonError = the HIP error code)
 *   devices       the HIP device index of every shard (an index may repeat); peerAccess[k]: the first device addresses device k's memory
 *   gathers / lastGatherMs / totalGatherMs   exchanges so far and their host-side wall time (submission to completion on the first device's stream) */
#define RTGPU_GATHER_NONE 0u
#define RTGPU_GATHER_PEER_KERNEL 1u
#define RTGPU_GATHER_STAGED_COPY 2u
typedef struct RtMultiInfo
{
    uint32_t numDevices, gatherMode, gatherReason;
    int32_t  reasonDevice, reasonError;
    int32_t  devices[16];
    uint32_t peerAccess[16];
    uint32_t reserved;
    uint64_t gathers;
    double   lastGatherMs, totalGatherMs;
} RtMultiInfo;
int rtgpu_get_multi_info(RtgpuContext* ctx, RtMultiInfo* out);

#ifdef __cplusplus
}
#endif

#endif /* RTGPU_H */
