"""`python -m pyrite_amd project.lua` -- what `pyrite project.lua` does for a project with the `simple` renderer
(pyrite/src/main.rs:46-330): load the project file, render it on the GPU, develop the film with the project's `image.filter`
/ `image.white`, and write `render.png` next to the project file (main.rs:180-184).

    python -m pyrite_amd path/to/project.lua [-o out.png] [--seed N] [--device D] [--spp N] [--size WxH]
                         [--pass-samples N] [--preview PATH] [--preview-every SECONDS] [--noise]
                         [--features PREFIX] [--features-grid N] [--hdr PATH] [--exposure EV|auto] [--tone clip|reinhard]
                         [--despeckle [K]] [--despeckle-radius R] [--denoise] [--denoise-radius N] [--upsample N] [--upsample-radius R]
                         [--glare [STRENGTH]] [--glare-levels N] [--glare-threshold T] [--lens-blur] [--lens-blur-radius R]
                         [--build host|device]

With --pass-samples, --preview or --noise the render runs as a progressive session (pyr_session_*): passes of N samples per pixel
over the whole image, the preview image rewritten from the live film every SECONDS or more (main.rs:261-299; developed on the GPU
with step 30, main.rs:270), and with --noise the largest and the median per-tile noise estimate printed after each preview. The
final image is the one the plain render writes.

With --features the first-hit feature pass (pyr_render_features, N x N sub-samples per pixel, default 1) runs after the render and
writes PREFIX_albedo.png, PREFIX_normal.png and PREFIX_depth.png.

With --hdr the final film is also written in linear light (linear sRGB, step 2, the project's filter and white): Radiance RGBE for
PATH.hdr, PFM for PATH.pfm. --exposure (stops, or auto: the median luminance to 0.18) and --tone (clip, or reinhard: the extended
Reinhard curve on luminance; alone it means --exposure auto) apply to the final PNG and to the previews. Without them the PNG is
the reference's hard clamp, byte for byte.

With --denoise the render runs as a session with two half films, in an even number of equal passes (two of half the samples when
--pass-samples is not given; an odd number of samples per pixel is refused), and the final PNG and the --hdr image are written
from the denoised linear image (pyr_session_denoised with the feature pass as its guide; window radius N, default 5): the PNG
through the tone curve, which without --exposure / --tone is the clip at exposure 1, the encoder of the plain PNG.

With --despeckle the render runs as a session with two half films, in an even number of equal passes as with --denoise, and the
fireflies of the two developed halves are clamped before anything else reads them (pyr_session_despeckled: a pixel more than K
spreads, default 6, above the median of its (2R+1)^2 window, R 1 or 2, default 2, in one half and not in the other): the order of
the stages is develop the halves, despeckle, denoise (with --denoise) or the mean of the halves, upsample, glare, tone. One line
with the pixels clamped in either half is printed. Previews are not despeckled.

With --upsample N the render runs at width/N x height/N with the project's camera -- N (2 to 8) must divide both -- and the final
image, of the project's size, is its linear image (the denoised one with --denoise) upsampled under the guidance of the first-hit
feature pass at both sizes (pyr_image_upsample: albedo, normals, depths and material ids; tent radius R, 1 to 3, default 1): after
the denoiser, before the glare and the tone curve. The --hdr image is the upsampled one; previews keep the low size.

With --glare the final image takes the linear path (the denoised image with --denoise) and the glare of a lens or an eye is added
to it (pyr_image_glare: STRENGTH of every pixel's light, default 0.1, spread over N blurs of doubling width, default 6; with
--glare-threshold T only what lies above the luminance T): before the statistics of an automatic exposure are taken and before the
tone curve, which without --exposure / --tone is the clip at exposure 1. The --hdr image is the glared one. Previews have no glare.

With --lens-blur the frame is rendered with the project camera's aperture set to 0 -- a pinhole, so that the image agrees with the
feature pass that steers --denoise and --upsample -- and the camera's own focus_distance and aperture are applied afterwards by a
filter that reads the depth of the full-size feature records (pyr_image_lens_blur; circles of confusion of at most R pixels, 1 to
16, default 8): after --despeckle, --denoise and --upsample, before --glare and the tone curve. What is in focus and out of every
blur's reach keeps the pinhole frame's values. The --hdr image is the blurred one; previews show the pinhole.

With --build the acceleration structure is built by the named builder (host: one CPU thread, the default; device: the same tree from
the GPU, pyr_scene_create_with) and one line with the builder used and the stage times of scene creation goes to stderr."""
import argparse
import os
import sys
import time


DEFAULT_PASS_SAMPLES = 256  # passes of a render with a preview when --pass-samples is not given: the smallest that cost nothing on C3


def progressive_flag_problem(pass_samples, preview, preview_every, noise):
    """What is wrong with the progressive flags, in the words pyrite_host_tool uses too, or None."""
    if pass_samples is not None and pass_samples < 1:
        return "--pass-samples must be at least 1"
    if not preview_every >= 0:
        return "--preview-every must not be negative"
    if noise and not preview:
        return "--noise needs --preview"
    return None


def render_progressive(r, cam, world, film, args, image, on_status):
    """The render as a session: passes, previews, noise. Returns the final host Film."""
    import numpy as np

    from .develop import save_png

    pass_samples = args.pass_samples or (r.pixel_samples // 2 if args.denoise or args.despeckle_params is not None else DEFAULT_PASS_SAMPLES)
    with r.session((film.width, film.height), cam, world, halves=args.noise or args.denoise or args.despeckle_params is not None, device=args.device) as s:
        on_status(0, "Rendering")
        last_image = time.monotonic()  # main.rs:241
        while s.samples_done < r.pixel_samples:
            s.render(pass_samples)
            s.sync()
            on_status(s.samples_done * 100 // r.pixel_samples, "Rendering")
            if args.preview and time.monotonic() - last_image >= args.preview_every:
                save_png(args.preview, s.preview(30.0, filter=image.get("filter"), white=image.get("white"), tone=args.tone_params))
                print("\nPreview updated (%d samples per pixel)" % s.samples_done)
                if args.noise and s.samples_done >= 2 * pass_samples:
                    noise = s.noise()
                    print("noise: largest tile %.4g, median tile %.4g" % (float(noise.max()), float(np.median(noise))))
                last_image = time.monotonic()
        if args.despeckle_params is not None:  # the halves cleaned, then the denoiser or their mean
            denoise = None if not args.denoise else {} if args.denoise_radius is None else {"radius": args.denoise_radius}
            args.denoised, _, _, counts = s.despeckled(2.0, filter=image.get("filter"), white=image.get("white"), denoise=denoise, **args.despeckle_params)
            print("\ndespeckle: %d pixels clamped in half A, %d in half B" % counts)
        elif args.denoise:
            params = {} if args.denoise_radius is None else {"radius": args.denoise_radius}
            args.denoised = s.denoised(2.0, filter=image.get("filter"), white=image.get("white"), **params)[0]
        return s.film()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m pyrite_amd", description=__doc__.split("\n\n")[0])
    ap.add_argument("project", help="project file (*.lua)")
    ap.add_argument("-o", "--output", default=None, help="image to write (default: render.png next to the project file)")
    ap.add_argument("--seed", type=int, default=None, help="RNG seed (default: from the clock; the reference seeds from OS entropy)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--spp", type=int, default=None, help="override renderer.pixel_samples")
    ap.add_argument("--size", default=None, help="override image size, WIDTHxHEIGHT")
    ap.add_argument("--pass-samples", type=int, default=None, help="render in passes of N samples per pixel (default with --preview: %d)" % DEFAULT_PASS_SAMPLES)
    ap.add_argument("--preview", default=None, metavar="PATH", help="image to rewrite from the live film while rendering")
    ap.add_argument("--preview-every", type=float, default=20.0, metavar="SECONDS", help="least time between two previews (default 20, main.rs:262)")
    ap.add_argument("--noise", action="store_true", help="print the largest and median per-tile noise estimate after each preview")
    ap.add_argument("--features", default=None, metavar="PREFIX", help="write PREFIX_albedo.png, PREFIX_normal.png and PREFIX_depth.png of the first hits")
    ap.add_argument("--features-grid", type=int, default=None, metavar="N", help="N x N sub-samples per pixel for --features (1 to 8, default 1)")
    ap.add_argument("--hdr", default=None, metavar="PATH", help="also write the image in linear light: PATH.hdr (Radiance RGBE) or PATH.pfm")
    ap.add_argument("--exposure", default=None, metavar="EV|auto", help="exposure of the PNG and the previews in stops, or auto")
    ap.add_argument("--tone", default=None, metavar="clip|reinhard", help="tone curve of the PNG and the previews (reinhard alone means --exposure auto)")
    ap.add_argument("--despeckle", nargs="?", const=str(6.0), default=None, metavar="K", help="clamp the fireflies of the two half images before they are denoised or averaged: spreads above the median at which a pixel is one (above 0, default 6)")
    ap.add_argument("--despeckle-radius", type=int, default=None, metavar="R", help="window radius of --despeckle (1 or 2, default 2)")
    ap.add_argument("--denoise", action="store_true", help="write the PNG and the --hdr image from the denoised linear image of two half films")
    ap.add_argument("--denoise-radius", type=int, default=None, metavar="N", help="window radius of --denoise (1 to 10, default 5)")
    ap.add_argument("--upsample", type=int, default=None, metavar="N", help="render at 1/N of the image size (2 to 8, N divides both sides) and upsample under the guidance of the feature pass")
    ap.add_argument("--upsample-radius", type=int, default=None, metavar="R", help="tent radius of --upsample in low-resolution pixels (1 to 3, default 1)")
    ap.add_argument("--glare", nargs="?", const=str(0.1), default=None, metavar="STRENGTH", help="add glare to the final image: the share of the light that is spread (above 0, at most 1; default 0.1)")
    ap.add_argument("--glare-levels", type=int, default=None, metavar="N", help="blurs of doubling width the glare sums (1 to 12, default 6)")
    ap.add_argument("--glare-threshold", type=float, default=None, metavar="T", help="luminance below which a pixel spreads nothing (default 0: every pixel spreads)")
    ap.add_argument("--lens-blur", action="store_true", help="render through a pinhole and apply the project camera's focus_distance and aperture as a filter over the feature records")
    ap.add_argument("--lens-blur-radius", type=int, default=None, metavar="R", help="largest circle of confusion of --lens-blur in pixels (1 to 16, default 8)")
    ap.add_argument("--build", default=None, choices=["host", "device"], help="who builds the BVH (default host); given, the stage times of scene creation go to stderr")
    args = ap.parse_args(argv)
    from .develop import denoise_flag_problem, despeckle_flag_problem, despeckle_from_flags, glare_flag_problem, glare_from_flags, lens_blur_flag_problem, tone_flag_problem, tone_from_flags, upsample_flag_problem, upsample_from_flags
    from .features import features_flag_problem

    problem = (progressive_flag_problem(args.pass_samples, args.preview, args.preview_every, args.noise) or features_flag_problem(args.features, args.features_grid)
               or tone_flag_problem(args.hdr, args.exposure, args.tone) or despeckle_flag_problem(args.despeckle, args.despeckle_radius)
               or denoise_flag_problem(args.denoise, args.denoise_radius)
               or upsample_flag_problem(args.upsample, args.upsample_radius) or glare_flag_problem(args.glare, args.glare_levels, args.glare_threshold)
               or lens_blur_flag_problem(args.lens_blur, args.lens_blur_radius))
    if problem:
        print("error: " + problem, file=sys.stderr)
        return 2

    args.tone_params = tone_from_flags(args.exposure, args.tone)
    args.despeckle_params = despeckle_from_flags(args.despeckle, args.despeckle_radius)
    args.glare_params = glare_from_flags(args.glare, args.glare_levels, args.glare_threshold)
    args.upsample_params = upsample_from_flags(args.upsample, args.upsample_radius)

    from . import lua_project, scenes
    from .develop import develop, develop_linear, glare, lens_blur, save_linear, save_png, tonemap, upsample

    project, base_dir = lua_project.load_project(args.project)
    if args.size:
        w, h = (int(x) for x in args.size.lower().split("x"))
        project.setdefault("image", {}).update(width=w, height=h)
    if args.spp:
        project["renderer"] = project["renderer"].with_(pixel_samples=args.spp)
    problem = despeckle_flag_problem(args.despeckle, args.despeckle_radius, int(project["renderer"].pixel_samples), args.pass_samples)
    problem = problem or denoise_flag_problem(args.denoise, args.denoise_radius, int(project["renderer"].pixel_samples), args.pass_samples)
    full_size = (int(project["image"]["width"]), int(project["image"]["height"]))
    problem = problem or upsample_flag_problem(args.upsample, args.upsample_radius, full_size)
    if problem:
        print("error: " + problem, file=sys.stderr)
        return 2
    if args.upsample:  # the render and everything before the upsample at 1/N of the size, under the same camera
        project["image"].update(width=full_size[0] // args.upsample, height=full_size[1] // args.upsample)
    seed = args.seed if args.seed is not None else int(time.time_ns() & 0x7FFFFFFFFFFFFFFF)
    world, cam, r, film = scenes.build(project, seed=seed, base_dir=base_dir)
    lens_cam = cam
    if args.lens_blur:  # the render, its guides and every filter before the lens see a pinhole
        from . import abi
        from .renderer import Camera

        cam = Camera(abi.PyrCamera.from_buffer_copy(lens_cam.c))
        cam.c.aperture = 0.0
    print("The scene contains %d objects." % (len(world.flat.tri_material) + len(world.flat.spheres) + len(world.flat.planes)))  # world.rs:251-254

    if args.build:
        world.scene(args.device, build=args.build)
        b = world.build_info(args.device)
        print("build: asked %s, used %s (fallback %d), %d levels, %d median splits, digest %016x; bounds %.2f tree %.2f finish %.2f collapse %.2f pack+upload %.2f total %.2f ms"
              % (args.build, "device" if b["builder_used"] == 1 else "host", b["fallback_reason"], b["levels"], b["median_splits"], b["tree_digest"],
                 b["bounds_ms"], b["tree_ms"], b["finish_ms"], b["collapse_ms"], b["pack_upload_ms"], b["total_ms"]), file=sys.stderr)

    def on_status(percent, message):
        print("\r%s... %3d %%" % (message, percent), end="", flush=True)

    t = time.time()
    image = project.get("image") or {}
    if args.pass_samples is not None or args.preview or args.noise or args.denoise or args.despeckle_params is not None:
        film = render_progressive(r, cam, world, film, args, image, on_status)
    else:
        r.render(film, cam, world, on_status=on_status, device=args.device)
    print("\rRendering... done in %.2f s (%.1f Msamples/s)" % (time.time() - t, film.width * film.height * r.pixel_samples / (time.time() - t) / 1e6))
    print("Saving final result...")  # main.rs:313
    linear = None
    if args.denoise or args.despeckle_params is not None:
        linear = args.denoised
    elif args.hdr or args.tone_params is not None or args.glare_params is not None or args.upsample or args.lens_blur:
        linear = develop_linear(film, "srgb", filter=image.get("filter"), white=image.get("white"), device=args.device)
    if args.upsample:  # after the denoiser, before the glare
        guides = [r.features(size, cam, world, device=args.device) for size in ((film.width, film.height), full_size)]
        low_albedo, albedo = (develop_linear(f.albedo, "srgb", filter=image.get("filter"), white=image.get("white"), device=args.device) for f in guides)
        linear = upsample(linear, args.upsample, albedo=albedo, pixels=guides[1].records, low_albedo=low_albedo, low_pixels=guides[0].records, device=args.device,
                          **args.upsample_params)
    if args.lens_blur:  # after the filters that read the guides, before the glare and the tone curve; the full-size records
        radius = {} if args.lens_blur_radius is None else {"max_radius": args.lens_blur_radius}
        linear = lens_blur(linear, r.features(full_size, cam, world, device=args.device).records, device=args.device, camera=lens_cam, **radius)
    if args.glare_params is not None:  # before the statistics of an automatic exposure, which tonemap takes
        linear = glare(linear, device=args.device, **args.glare_params)
    if args.tone_params is not None or args.denoise or args.despeckle_params is not None or args.glare_params is not None or args.upsample or args.lens_blur:
        rgb = tonemap(linear, args.tone_params, device=args.device)
    else:
        rgb = develop(film, filter=image.get("filter"), white=image.get("white"), device=args.device)
    out = args.output or os.path.join(base_dir, "render.png")
    save_png(out, rgb)
    print("wrote", out)
    if args.hdr:
        save_linear(args.hdr, linear)
        print("wrote", args.hdr)
    if args.features:
        from .features import write_feature_images

        write_feature_images(args.features, r.features(full_size, cam, world, grid=args.features_grid or 1, device=args.device),
                             filter=image.get("filter"), white=image.get("white"), device=args.device)
        print("wrote %s_albedo.png, %s_normal.png, %s_depth.png" % (args.features, args.features, args.features))
    return 0


if __name__ == "__main__":
    sys.exit(main())
