// Headless counterpart of the reference's Demo (Demo/Main.cpp:6-40 takes -w/--width, -h/--height, -s/--scene, --renderer,
// --data and opens a window): loads a JSON scene with helpers::LoadScene, renders N passes with the device "Path Tracer MIS"
// through the same rt::Viewport API the window loop uses (Demo.cpp: Resize -> SetRenderer -> Render per frame ->
// GetFrontBuffer) and writes the tone-mapped front buffer as a BMP.  The extra options are --passes, --depth, --output, --seed and
// --debug-pixel X,Y (prints the path behind that pixel of pass 0, what the reference's Demo shows for a picked pixel: Demo_UserInterface.cpp:197-272),
// --denoise [N] (the frame goes through N levels, default 5, of the a-trous filter before it is tone-mapped: rtgpu_denoise, rtgpu_postprocess_from)
// and --denoise-variance [N] (the same through the variance-guided filter over the film's two sum buffers: rtgpu_denoise_var),
// --guide-chain N beside either (the filter's guides follow every pixel's path through up to N mirror and glass vertices: rtgpu_set_guide_chain);
// --projection orthographic|panorama|fisheye (the frame is rendered along a table of primary rays built here from the scene file's camera transform, in
// place of the perspective camera: Viewport::SetLensSource, so the viewport's anti-aliasing applies to it; --projection-size S: the orthographic picture is 2 S world units wide, --projection-fov D: the
// fisheye's image circle spans D degrees; --aperture A --focal-distance F [--bokeh circle|hexagon|square]: the projection's rays pass a thin lens of radius A
// focused F along each ray; --denoise and --denoise-variance work with it: their guides follow the table);
// the environment variable RTGPU_DEVICES ("0,1,2,3" / "all") spreads the frame over several GPUs (Core/Rendering/Renderer.h).
#include "../Demo.h"
#include "../SceneLoader.h"
#include "../../Core/Rendering/Viewport.h"
#include "../../Core/Rendering/Renderer.h"
#include "../../Core/Rendering/PathTracerMIS.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

using namespace rt;

static bool SaveBMP(const char* path, const Bitmap& front)   // 24-bit, rows bottom-up like the BMP files the loader reads
{
    const uint32 w = front.GetWidth(), h = front.GetHeight(), row = (w * 3u + 3u) & ~3u;
    FILE* f = fopen(path, "wb");
    if (!f) return false;
#pragma pack(push, 2)
    struct { uint16 type; uint32 size; uint16 r1, r2; uint32 offBits; uint32 infoSize; int32 width, height; uint16 planes, bitCount; uint32 compression, sizeImage; int32 xppm, yppm; uint32 clrUsed, clrImportant; }
        hdr = { 0x4D42, 54u + row * h, 0, 0, 54, 40, (int32)w, (int32)h, 1, 24, 0, row * h, 2835, 2835, 0, 0 };
#pragma pack(pop)
    bool ok = fwrite(&hdr, sizeof(hdr), 1, f) == 1;
    std::string line(row, '\0');
    for (uint32 y = 0; ok && y < h; ++y)
    {
        const uint32* src = reinterpret_cast<const uint32*>(front.GetBytes() + (size_t)front.GetStride() * (h - 1u - y));
        for (uint32 x = 0; x < w; ++x) { line[3 * x + 0] = (char)(src[x] & 255u); line[3 * x + 1] = (char)((src[x] >> 8) & 255u); line[3 * x + 2] = (char)((src[x] >> 16) & 255u); }
        ok = fwrite(line.data(), row, 1, f) == 1;
    }
    fclose(f);
    return ok;
}

// The path of pixel (x, y) of the pass `params` (rtgpu_record_paths), one line per vertex and the reason it ended
static bool PrintPixelPath(IRenderer* renderer, const RtPassParams& params, uint32 x, uint32 y)
{
    static const char* const reasons[] = { "None", "HitBackground", "HitLight", "Depth", "Throughput", "NoSampledEvent", "RussianRoulette" };   // PathTerminationReason
    PathTracerMIS* pt = dynamic_cast<PathTracerMIS*>(renderer);
    if (!pt || !pt->UploadScene()) { fprintf(stderr, "--debug-pixel: the renderer has no device context\n"); return false; }
    const uint32 pixel[2] = { x, y };
    std::vector<RtPathVertex> vertices(params.maxRayDepth + 1u);
    RtPathInfo info;
    if (rtgpu_record_paths(pt->GetDeviceContext(), &params, pixel, 1u, (uint32)vertices.size(), vertices.data(), &info) != RTGPU_OK)
    {
        fprintf(stderr, "--debug-pixel: %s\n", rtgpu_last_error());
        return false;
    }
    printf("pixel (%u, %u), pass %u: %u vertices, %s, radiance (%g, %g, %g)\n", x, y, params.passIndex, info.numVertices,
           info.terminationReason < 7u ? reasons[info.terminationReason] : "?", (double)info.radiance[0], (double)info.radiance[1], (double)info.radiance[2]);
    for (uint32 i = 0; i < info.numVertices && i < vertices.size(); ++i)
    {
        const float* w = vertices[i].w;
        uint32 object, subObject, event;
        memcpy(&object, w + 6, 4); memcpy(&subObject, w + 7, 4); memcpy(&event, w + 26, 4);
        printf("  %u: origin (%g, %g, %g) dir (%g, %g, %g)", i, (double)w[0], (double)w[1], (double)w[2], (double)w[3], (double)w[4], (double)w[5]);
        if (object == RT_INVALID_OBJECT) printf(" miss");
        else printf(" object %u sub %s%u distance %g at (%g, %g, %g) normal (%g, %g, %g)", object, subObject == RT_LIGHT_OBJECT ? "light " : "", subObject == RT_LIGHT_OBJECT ? 0u : subObject,
                    (double)w[8], (double)w[11], (double)w[12], (double)w[13], (double)w[14], (double)w[15], (double)w[16]);
        printf(" throughput (%g, %g, %g) event %u\n", (double)w[22], (double)w[23], (double)w[24], event);
    }
    return true;
}

// The front buffer of the frame after `levels` levels of the a-trous filter (rtgpu_denoise guided by the first hits of one more pass's primary rays,
// then the viewport's post-process over the filtered image).  `variance`: rtgpu_denoise_var, the variance-guided filter.  guideChain >= 0: the guides are
// those of the paths' guide vertices (rtgpu_set_guide_chain)
static bool DenoisedFrontBuffer(Viewport& viewport, const Camera& camera, IRenderer* renderer, uint32 levels, bool variance, int guideChain, Bitmap& front)
{
    PathTracerMIS* pt = dynamic_cast<PathTracerMIS*>(renderer);
    if (!pt || !pt->UploadScene()) { fprintf(stderr, "--denoise: the renderer has no device context\n"); return false; }
    if (guideChain >= 0)
    {
        RtAovChain chain; memset(&chain, 0, sizeof(chain));
        chain.maxChain = (uint32)guideChain;
        if (rtgpu_set_guide_chain(pt->GetDeviceContext(), &chain) != RTGPU_OK) { fprintf(stderr, "--guide-chain: %s\n", rtgpu_last_error()); return false; }
    }
    const uint32 w = viewport.GetWidth(), h = viewport.GetHeight(), passes = viewport.GetProgress().passesFinished ? viewport.GetProgress().passesFinished : 1u;
    RtPassParams guide;
    if (!viewport.NextPassParams(camera, guide)) return false;
    RtDenoiseParams dp; memset(&dp, 0, sizeof(dp));
    dp.iterations = levels; dp.flags = RT_DENOISE_DEMODULATE; dp.colorScale = 1.0f / (float)passes;
    dp.sigmaColor = 2.0f; dp.sigmaNormal = 0.25f; dp.sigmaPlane = 0.1f;
    RtDenoiseVarParams dv; memset(&dv, 0, sizeof(dv));
    dv.iterations = levels; dv.flags = RT_DENOISE_DEMODULATE; dv.colorScale = dp.colorScale;
    dv.sigmaLum = 4.0f; dv.sigmaNormal = dp.sigmaNormal; dv.sigmaPlane = dp.sigmaPlane; dv.varianceFloor = 1e-10f;
    std::vector<float> image((size_t)w * h * 3u);
    const PostprocessParams& pp = viewport.GetPostprocessParams();
    RtPostprocessParams p; memset(&p, 0, sizeof(p));
    memcpy(p.colorFilter, &pp.colorFilter, 16);
    p.exposure = pp.exposure; p.contrast = pp.contrast; p.saturation = pp.saturation; p.ditheringStrength = pp.ditheringStrength; p.bloomFactor = pp.bloomFactor;
    p.tonemapper = (uint32)pp.tonemapper; p.numPasses = 1u; p.ditherSeed = passes;   // (the image is averaged already: colorScale)
    Bitmap::InitData init;
    init.width = w; init.height = h; init.format = Bitmap::Format::B8G8R8A8_UNorm; init.linearSpace = false;   // as Viewport::GetFrontBuffer makes it
    if (!front.Init(init)) return false;
    if ((variance ? rtgpu_denoise_var(pt->GetDeviceContext(), &dv, &guide, image.data(), nullptr) : rtgpu_denoise(pt->GetDeviceContext(), &dp, &guide, image.data())) != RTGPU_OK ||
        rtgpu_postprocess_from(pt->GetDeviceContext(), &p, image.data(), reinterpret_cast<uint32*>(front.GetBytes())) != RTGPU_OK)
    {
        fprintf(stderr, "--denoise: %s\n", rtgpu_last_error());
        return false;
    }
    return true;
}

// The table of --projection: one lens ray per pixel (RtLensRay), row 0 the top of the picture, from the camera's transform (rows: right, up, forward,
// position).  orthographic: parallel rays along forward, the picture 2 * size wide; panorama: equirectangular, the centre column looks forward and the rows
// sweep from straight up to straight down; fisheye: equidistant, fovDegrees across the circle inscribed in the shorter side, the axis ray outside it.
// The stored ray is the projection's at the pixel's centre; its footprint -- what the viewport's anti-aliasing offset moves it by, per pixel of offset -- is
// the projection's own central difference over the pixel ((ray at +1/2) - (ray at -1/2), x to the right, y up); the lens plane is spanned by U = up x d,
// normalised, and V = d x U (orthographic: right and up; at a direction parallel to up: U = right), its aperture and focal distance the caller's.
static std::vector<RtLensRay> ProjectionTable(const std::string& projection, const RtCamera& camera, uint32 width, uint32 height, double size, double fovDegrees,
                                              double aperture, double focalDistance)
{
    const double pi = 3.14159265358979323846;
    const float* m = camera.localToWorld;
    const double right[3] = { m[0], m[1], m[2] }, up[3] = { m[4], m[5], m[6] }, forward[3] = { m[8], m[9], m[10] }, position[3] = { m[12], m[13], m[14] };
    std::vector<RtLensRay> table((size_t)width * height);
    const double shorter = width < height ? width : height;
    // the projection's ray through pixel (x, y) at sample offset (sx, sy) from its centre
    auto rayAt = [&](uint32 x, uint32 y, double sx, double sy, double o[3], double d[3])
    {
        const double u = (x + 0.5 + sx) / width, v = (height - 1u - y + 0.5 + sy) / height;   // film coordinates: v up
        for (int k = 0; k < 3; ++k) o[k] = position[k];
        double cr = 0.0, cu = 0.0, cf = 1.0;   // the direction's coordinates along right, up, forward
        if (projection == "orthographic")
        {
            const double px = (2.0 * u - 1.0) * size, py = (2.0 * v - 1.0) * size * height / width;
            for (int k = 0; k < 3; ++k) o[k] += px * right[k] + py * up[k];
        }
        else if (projection == "panorama")
        {
            const double azimuth = (u - 0.5) * 2.0 * pi, elevation = (v - 0.5) * pi;
            cf = cos(elevation) * cos(azimuth); cr = cos(elevation) * sin(azimuth); cu = sin(elevation);
        }
        else   // fisheye
        {
            const double px = (2.0 * u - 1.0) * width / shorter, py = (2.0 * v - 1.0) * height / shorter, r = sqrt(px * px + py * py);
            if (r > 0.0 && r <= 1.0)
            {
                const double theta = r * 0.5 * fovDegrees * pi / 180.0;
                cf = cos(theta); cr = sin(theta) * px / r; cu = sin(theta) * py / r;
            }
        }
        for (int k = 0; k < 3; ++k) d[k] = cr * right[k] + cu * up[k] + cf * forward[k];
    };
    auto cross = [](const double a[3], const double b[3], double out[3]) { out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0]; };
    auto normalise = [](double a[3]) { const double l = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); if (l > 0.0) for (int k = 0; k < 3; ++k) a[k] /= l; return l; };
    for (uint32 y = 0; y < height; ++y)
        for (uint32 x = 0; x < width; ++x)
        {
            double o[3], d[3], op[3], dp[3], om[3], dm[3];
            RtLensRay& ray = table[(size_t)y * width + x];
            memset(&ray, 0, sizeof(ray));
            rayAt(x, y, 0.0, 0.0, o, d);
            for (int k = 0; k < 3; ++k) { ray.origin[k] = (float)o[k]; ray.direction[k] = (float)d[k]; }
            rayAt(x, y, 0.5, 0.0, op, dp); rayAt(x, y, -0.5, 0.0, om, dm);
            for (int k = 0; k < 3; ++k) { ray.dOriginDsx[k] = (float)(op[k] - om[k]); ray.dDirectionDsx[k] = (float)(dp[k] - dm[k]); }
            rayAt(x, y, 0.0, 0.5, op, dp); rayAt(x, y, 0.0, -0.5, om, dm);
            for (int k = 0; k < 3; ++k) { ray.dOriginDsy[k] = (float)(op[k] - om[k]); ray.dDirectionDsy[k] = (float)(dp[k] - dm[k]); }
            double unit[3] = { d[0], d[1], d[2] }, lensU[3], lensV[3];
            normalise(unit);
            cross(up, unit, lensU);
            if (normalise(lensU) < 1e-6)   // d along up: the right axis, its part along d removed
            {
                const double along = right[0] * unit[0] + right[1] * unit[1] + right[2] * unit[2];
                for (int k = 0; k < 3; ++k) lensU[k] = right[k] - along * unit[k];
                normalise(lensU);
            }
            cross(unit, lensU, lensV);
            for (int k = 0; k < 3; ++k) { ray.lensU[k] = (float)lensU[k]; ray.lensV[k] = (float)lensV[k]; }
            ray.aperture = (float)aperture; ray.focalDistance = (float)focalDistance;
        }
    return table;
}

int main(int argc, char* argv[])
{
    uint32 width = 1280, height = 720, passes = 64, depth = 20;
    bool debugPixel = false; uint32 debugX = 0, debugY = 0;
    uint32 denoiseLevels = 0; bool denoiseVariance = false; int guideChain = -1;
    std::string scenePath, rendererName = "Path Tracer MIS", output = "out.bmp";
    unsigned long long seed = 0; bool haveSeed = false;
    std::string projection; double projectionSize = 5.0, projectionFov = 180.0;
    double lensAperture = 0.0, lensFocalDistance = 1.0; bool haveLens = false; uint32 lensBokeh = 0;
    for (int i = 1; i < argc; ++i)
    {
        const std::string a = argv[i];
        auto value = [&](const char* name) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", name); exit(2); } return argv[++i]; };
        if (a == "-w" || a == "--width") width = (uint32)atoi(value("--width"));
        else if (a == "-h" || a == "--height") height = (uint32)atoi(value("--height"));
        else if (a == "-s" || a == "--scene") scenePath = value("--scene");
        else if (a == "--renderer") rendererName = value("--renderer");
        else if (a == "--data") gOptions.dataPath = value("--data");
        else if (a == "--passes") passes = (uint32)atoi(value("--passes"));
        else if (a == "--depth") depth = (uint32)atoi(value("--depth"));
        else if (a == "--output") output = value("--output");
        else if (a == "--seed") { seed = strtoull(value("--seed"), nullptr, 10); haveSeed = true; }
        else if (a == "--debug-pixel") { if (sscanf(value("--debug-pixel"), "%u,%u", &debugX, &debugY) != 2) { fprintf(stderr, "--debug-pixel takes X,Y\n"); return 2; } debugPixel = true; }
        else if (a == "--denoise" || a == "--denoise-variance")
        {
            denoiseLevels = 5;   // the level count is optional
            denoiseVariance = a == "--denoise-variance";
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') denoiseLevels = (uint32)atoi(argv[++i]);
            if (denoiseLevels < 1 || denoiseLevels > 8) { fprintf(stderr, "%s takes 1..8 levels\n", a.c_str()); return 2; }
        }
        else if (a == "--guide-chain")
        {
            guideChain = atoi(value("--guide-chain"));
            if (guideChain < 0 || guideChain > (int)RT_AOV_CHAIN_MAX) { fprintf(stderr, "--guide-chain takes 0..%u vertices\n", RT_AOV_CHAIN_MAX); return 2; }
        }
        else if (a == "--projection")
        {
            projection = value("--projection");
            if (projection != "orthographic" && projection != "panorama" && projection != "fisheye") { fprintf(stderr, "--projection takes orthographic, panorama or fisheye\n"); return 2; }
        }
        else if (a == "--projection-size") { projectionSize = atof(value("--projection-size")); if (!(projectionSize > 0.0)) { fprintf(stderr, "--projection-size takes a positive half width\n"); return 2; } }
        else if (a == "--projection-fov") { projectionFov = atof(value("--projection-fov")); if (!(projectionFov > 0.0 && projectionFov <= 360.0)) { fprintf(stderr, "--projection-fov takes 0..360 degrees\n"); return 2; } }
        else if (a == "--aperture") { lensAperture = atof(value("--aperture")); haveLens = true; if (!(lensAperture >= 0.0)) { fprintf(stderr, "--aperture takes a lens radius >= 0\n"); return 2; } }
        else if (a == "--focal-distance") { lensFocalDistance = atof(value("--focal-distance")); haveLens = true; if (!(lensFocalDistance > 0.0)) { fprintf(stderr, "--focal-distance takes a positive distance\n"); return 2; } }
        else if (a == "--bokeh")
        {
            const std::string shape = value("--bokeh");
            haveLens = true;
            if (shape == "circle") lensBokeh = 0; else if (shape == "hexagon") lensBokeh = 1; else if (shape == "square") lensBokeh = 2;
            else { fprintf(stderr, "--bokeh takes circle, hexagon or square\n"); return 2; }
        }
        else { fprintf(stderr, "usage: rt_demo -s scene.json [--data dir/] [-w W] [-h H] [--passes N] [--depth D] [--renderer name] [--output out.bmp] [--seed N] [--debug-pixel X,Y] [--denoise [N]] [--denoise-variance [N]] [--guide-chain N] [--projection orthographic|panorama|fisheye] [--projection-size S] [--projection-fov DEGREES] [--aperture A] [--focal-distance F] [--bokeh circle|hexagon|square]\n"); return 2; }
    }
    if (guideChain >= 0 && !denoiseLevels) { fprintf(stderr, "--guide-chain steers the denoiser's guides: it needs --denoise or --denoise-variance\n"); return 2; }
    if (haveLens && projection.empty()) { fprintf(stderr, "--aperture, --focal-distance and --bokeh give a --projection its thin lens (the scene file sets the perspective camera's)\n"); return 2; }
    if (scenePath.empty()) { fprintf(stderr, "no scene given (-s scene.json)\n"); return 2; }

    Scene scene;
    Camera camera;
    if (!helpers::LoadScene(scenePath, scene, camera)) return 1;
    if (!scene.BuildBVH()) return 1;
    camera.SetPerspective((float)width / (float)height, camera.mFieldOfView);

    Viewport viewport;
    RenderingParams params;
    params.maxRayDepth = depth;
    if (haveSeed) viewport.SetSeed(seed);   // reproducible frames (the reference seeds its generators from the clock)
    if (!viewport.SetRenderingParams(params) || !viewport.Resize(width, height)) return 1;
    RendererPtr renderer = CreateRenderer(rendererName, scene);
    if (!renderer) { fprintf(stderr, "renderer '%s' is not available (no GPU?)\n", rendererName.c_str()); return 1; }
    if (!viewport.SetRenderer(renderer)) return 1;
    viewport.Reset();
    if (!projection.empty())
    {
        RtCamera desc;
        if (!camera.GetDesc(desc)) return 1;
        // one lens table for the whole run: the viewport's anti-aliasing offsets and the lens draws are applied to it on the device, pass after pass
        const std::vector<RtLensRay> table = ProjectionTable(projection, desc, width, height, projectionSize, projectionFov, lensAperture, lensFocalDistance);
        const RtLensSourceParams lens = { haveLens ? 1u : 0u, lensBokeh };
        if (!viewport.SetLensSource(table.data(), table.size(), lens)) return 1;
        printf("projection: %s, %zu primary rays from the scene's camera transform\n", projection.c_str(), table.size());
        if (haveLens) printf("lens: aperture %g, focal distance %g, bokeh shape %u\n", lensAperture, lensFocalDistance, lensBokeh);
    }

    const auto t0 = std::chrono::steady_clock::now();
    uint32 rendered = 0;
    if (debugPixel)
    {
        // pass 0 with its constants in hand: recorded for the pixel, then rendered as Render() would have
        RtPassParams first;
        if (!viewport.NextPassParams(camera, first) || !PrintPixelPath(renderer.get(), first, debugX, debugY)) return 1;
        if (passes > 0) { if (!renderer->RenderPass(first)) return 1; viewport.FinishPass(); rendered = 1; }
    }
    for (uint32 i = rendered; i < passes; ++i) if (!viewport.Render(camera)) return 1;
    const RayTracingCounters counters = viewport.GetTotalCounters();   // synchronises
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%u passes of %ux%u in %.3f s: %.1f Msamples/s (%llu paths x bounces, %llu shadow rays), average error %g\n", passes, width, height, seconds,
           (double)counters.numRays / seconds / 1.0e6, (unsigned long long)counters.numRays, (unsigned long long)counters.numShadowRays,
           (double)viewport.GetProgress().averageError);
    Bitmap denoised;
    if (denoiseLevels && !DenoisedFrontBuffer(viewport, camera, renderer.get(), denoiseLevels, denoiseVariance, guideChain, denoised)) return 1;
    if (denoiseLevels) printf("denoised: %u levels of the %sa-trous filter\n", denoiseLevels, denoiseVariance ? "variance-guided " : "");
    if (denoiseLevels && guideChain >= 0) printf("guides: chains of at most %d mirror and glass vertices\n", guideChain);
    if (!SaveBMP(output.c_str(), denoiseLevels ? denoised : viewport.GetFrontBuffer())) { fprintf(stderr, "cannot write %s\n", output.c_str()); return 1; }
    printf("wrote %s\n", output.c_str());
    return 0;
}
