// raytracer — drop-in command line of the reference (src/main.cpp:230-413):
//   ./raytracer --path scene.scn --output image.ppm [--width i] [--height i] [--fov f]
//               [--gillum n] [--jsample g] [--depth d] [--parallel true|false] [--shadow]
// Flags are matched by strcmp anywhere in argv and unknown tokens are ignored,
// messages and the exit-status-0 convention follow the reference.  New,
// non-colliding flags: --seed u64 (counter-RNG key; the reference seeds rand()
// with time(0)), --device i, --quiet (no per-line scene echo), --gpus N, --strict-scn,
// --scn-fog, --scn-spot (spot_light lines parsed and shaded: include/skr.h SKR_SCN_SPOT), --light-radius R (every point and spot light a sphere of radius R: include/skr.h skr_scene_set_light_radii), --aperture A [--focus F] (a thin lens: depth of field, include/skr.h skr_scene_set_lens; --focus alone has no effect), --scn-motion [--shutter S] (velocity lines parsed, the spheres move while the shutter is open: motion blur, include/skr.h skr_scene_set_sphere_velocities; --shutter without velocities has no effect), --envmap FILE.pfm (a square colour PFM as the scene's environment: rays that miss return it, an image-based background and GI light, include/skr.h skr_scene_set_environment), --scn-texture (texture lines parsed, the spheres that follow carry the image as their albedo: include/skr.h SKR_SCN_TEXTURE), --scn-emission (emission lines parsed, the spheres that follow glow: include/skr.h SKR_SCN_EMISSION), --scn-fov, --shade-triangles, --sphere-tree (the culled sphere walk, spheres in HBM: any sphere count), --triangle-shadows (needs --shade-triangles and --shadow to have an effect; accepted without them), --legacy-reflect, --progressive K [--progressive-every M], --format ppm|png|pfm, --denoise L,
// --adaptive T [--adaptive-min K] [--adaptive-max N] [--adaptive-denoise L].
// The frame itself is rendered by libskr on the GPU; there is no CPU path here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "skr.h"

int main(int argc, char *argv[])
{
	skr_options option;
	skr_options_default(&option);
	const char *path = nullptr, *output = nullptr;
	bool visual = true; // utils.h:29; kept for compatibility: there is no SDL viewer, both values render on the GPU
	bool quiet = false;
	int device = 0, gpus = 1;
	bool strict_scn = false, width_given = false, height_given = false, depth_given = false; // --strict-scn (new)
	bool scn_spot = false; // --scn-spot (new: DESIGN.md 8.12)
	bool radius_given = false; // --light-radius R (new: DESIGN.md 8.13)
	float light_radius = 0.0f;
	bool aperture_given = false; // --aperture A [--focus F] (new: DESIGN.md 8.15)
	float aperture = 0.0f, focus = 1.0f;
	bool scn_motion = false;     // --scn-motion (new: DESIGN.md 8.16; include/skr.h SKR_SCN_MOTION)
	bool scn_texture = false;    // --scn-texture (new: DESIGN.md 8.18; include/skr.h SKR_SCN_TEXTURE)
	bool scn_emission = false;   // --scn-emission (new: DESIGN.md 8.19; include/skr.h SKR_SCN_EMISSION)
	bool shutter_given = false;  // --shutter S
	float shutter = 1.0f;
	const char *envmap = nullptr; // --envmap FILE.pfm (new: DESIGN.md 8.17; include/skr.h skr_scene_set_environment)
	bool scn_fog = false, scn_fov = false, fov_given = false; // --scn-fog, --scn-fov (new: DESIGN.md "Spherical fog", "Camera half-angle")
	bool triangle_shadows = false; // --triangle-shadows (new: include/skr.h SKR_SCN_TRIANGLE_SHADOWS)
	bool sphere_tree = false;      // --sphere-tree (new: include/skr.h SKR_SCN_SPHERE_TREE)
	bool sharded = false; // --gpus given (even --gpus 1): the frame goes through the multi-GPU path
	uint32_t tile_rows = 8;
	int denoise = 0;  // --denoise L: the frame filtered by L iterations of the denoiser (include/skr.h skr_render_denoised_host)
	bool denoised = false;
	bool adaptive = false; // --adaptive T [--adaptive-min K] [--adaptive-max N]: passes per pixel while it is still noisy (include/skr.h skr_render_adaptive)
	skr_adaptive adapt;
	skr_adaptive_default(&adapt);
	int adaptive_denoise = 0; // --adaptive-denoise L (with --adaptive): the adaptive frame filtered under its measured variance (skr_render_adaptive_denoised_host)
	bool adaptive_denoised = false;
	uint32_t progressive_every = 0; // --progressive-every M: the output file is rewritten after every M passes (the headless "viewer")
	const char *format = "ppm";     // --format ppm | png | pfm (new; the reference writes P6 whatever the name says)

	for(int i = 0; i < argc; i++)
	{
		const bool has_next = i + 1 < argc;
		if(!strcmp(argv[i], "--gillum"))
		{
			if(has_next)
			{
				option.monte_carlo = 1;
				option.num_path_traces = atoi(argv[i + 1]);
			}
			else std::cerr << "gillum takes an int after flag for the number of paths traced" << std::endl; // main.cpp:258: warns, goes on
		}
		if(!strcmp(argv[i], "--fov"))
		{
			if(!has_next)
			{
				std::cerr << "fov takes a float (degrees) after flag for the field of view" << std::endl;
				return 0;
			}
			option.fov = (float) atof(argv[i + 1]);
			fov_given = true;
		}
		if(!strcmp(argv[i], "--jsample"))
		{
			if(!has_next)
			{
				std::cerr << "jsample takes an int after flag for the supersampling grid size" << std::endl;
				return 0;
			}
			option.grid_size = atoi(argv[i + 1]);
		}
		if(!strcmp(argv[i], "--width"))
		{
			if(!has_next)
			{
				std::cerr << "width takes an int after flag for the width" << std::endl;
				return 0;
			}
			option.width = atoi(argv[i + 1]);
			width_given = true;
		}
		if(!strcmp(argv[i], "--height"))
		{
			if(!has_next)
			{
				std::cerr << "height takes an int after flag for the width" << std::endl;
				return 0;
			}
			option.height = atoi(argv[i + 1]);
			height_given = true;
		}
		if(!strcmp(argv[i], "--depth"))
		{
			if(!has_next || atoi(argv[i + 1]) <= 0)
			{
				std::cerr << "depth takes a positive int after flag for the max depth" << std::endl;
				return 0;
			}
			option.max_depth = atoi(argv[i + 1]);
			depth_given = true;
		}
		if(!strcmp(argv[i], "--parallel"))
		{
			if(has_next && !strcmp(argv[i + 1], "true")) visual = false;
			if(has_next && !strcmp(argv[i + 1], "false")) visual = true;
		}
		if(!strcmp(argv[i], "--path"))
		{
			if(!has_next)
			{
				std::cerr << "path must be passed after --path" << std::endl;
				return 0;
			}
			path = argv[i + 1];
		}
		if(!strcmp(argv[i], "--output"))
		{
			if(!has_next)
			{
				std::cerr << "output path must be passed after --output" << std::endl;
				return 0;
			}
			output = argv[i + 1];
		}
		if(!strcmp(argv[i], "--shadow")) option.use_shadows = 1;
		if(!strcmp(argv[i], "--seed") && has_next) option.seed = strtoull(argv[i + 1], nullptr, 10);
		if(!strcmp(argv[i], "--device") && has_next) device = atoi(argv[i + 1]);
		if(!strcmp(argv[i], "--gpus") && has_next) { gpus = atoi(argv[i + 1]) > 0 ? atoi(argv[i + 1]) : 1; sharded = true; }           // new: the frame sharded over the first N devices
		if(!strcmp(argv[i], "--tile-rows") && has_next) tile_rows = (uint32_t) (atoi(argv[i + 1]) > 0 ? atoi(argv[i + 1]) : 8);
		if(!strcmp(argv[i], "--quiet")) quiet = true;
		if(!strcmp(argv[i], "--strict-scn")) strict_scn = true;
		if(!strcmp(argv[i], "--scn-spot")) scn_spot = true;                 // new: spot_light lines parsed and shaded (include/skr.h SKR_SCN_SPOT)
		if(!strcmp(argv[i], "--light-radius") && has_next) { light_radius = strtof(argv[i + 1], nullptr); radius_given = true; } // new: every point and spot light a sphere of radius R
		if(!strcmp(argv[i], "--scn-motion")) scn_motion = true;             // new: velocity lines parsed, the spheres move while the shutter is open (include/skr.h SKR_SCN_MOTION)
		if(!strcmp(argv[i], "--scn-texture")) scn_texture = true;           // new: texture lines parsed, the spheres that follow carry the image (include/skr.h SKR_SCN_TEXTURE)
		if(!strcmp(argv[i], "--scn-emission")) scn_emission = true;         // new: emission lines parsed, the spheres that follow glow (include/skr.h SKR_SCN_EMISSION)
		if(!strcmp(argv[i], "--shutter") && has_next) { shutter = strtof(argv[i + 1], nullptr); shutter_given = true; } // new: the shutter S (default 1); no effect without velocities
		if(!strcmp(argv[i], "--envmap") && has_next) envmap = argv[i + 1];     // new: the scene's environment, a square colour PFM
		if(!strcmp(argv[i], "--aperture") && has_next) { aperture = strtof(argv[i + 1], nullptr); aperture_given = true; } // new: a thin lens of aperture radius A
		if(!strcmp(argv[i], "--focus") && has_next) focus = strtof(argv[i + 1], nullptr);                                 // ... in focus at t = F of the primary rays
		if(!strcmp(argv[i], "--scn-fog")) scn_fog = true;                   // new: spherical_fog lines parsed and shaded (include/skr.h SKR_SCN_FOG)
		if(!strcmp(argv[i], "--scn-fov")) scn_fov = true;                   // new: fov = 2 x the camera line's half_height_angle unless --fov is given
		if(!strcmp(argv[i], "--shade-triangles")) option.shade_triangles = 1; // new: triangles as surfaces (include/skr.h skr_options)
		if(!strcmp(argv[i], "--sphere-tree")) sphere_tree = true;              // new: the culled sphere walk, spheres in HBM: any sphere count, the same image
		if(!strcmp(argv[i], "--triangle-shadows")) triangle_shadows = true;    // new: triangles cast shadows; needs --shade-triangles and --shadow to have an effect
		if(!strcmp(argv[i], "--legacy-reflect")) option.legacy_reflect = 1;   // new: the reflection / refraction code behind raytrace.h:44's early return
		if(!strcmp(argv[i], "--progressive") && has_next) option.progressive_passes = atoi(argv[i + 1]) > 1 ? atoi(argv[i + 1]) : 1; // new: mean of K frames, seeds seed..seed+K-1
		if(!strcmp(argv[i], "--progressive-every") && has_next) progressive_every = (uint32_t) (atoi(argv[i + 1]) > 0 ? atoi(argv[i + 1]) : 0);
		if(!strcmp(argv[i], "--format") && has_next) format = argv[i + 1];
		if(!strcmp(argv[i], "--denoise") && has_next) { denoise = atoi(argv[i + 1]); denoised = true; } // new: edge-aware denoiser, L iterations
		if(!strcmp(argv[i], "--adaptive") && has_next) { adapt.threshold = strtof(argv[i + 1], nullptr); adaptive = true; } // new: adaptive sampling
		if(!strcmp(argv[i], "--adaptive-min") && has_next) adapt.min_passes = atoi(argv[i + 1]);
		if(!strcmp(argv[i], "--adaptive-max") && has_next) adapt.max_passes = atoi(argv[i + 1]);
		if(!strcmp(argv[i], "--adaptive-denoise") && has_next) { adaptive_denoise = atoi(argv[i + 1]); adaptive_denoised = true; } // new: the two together
	}
	if(!path)
	{
		std::cerr << "no scene file was passed. Pass with --path path_to_scn" << std::endl;
		return 0;
	}
	if(!output)
	{
		std::cerr << "no output destination was passed. Pass with --output destination_path.ppm" << std::endl;
		return 0;
	}
	if(radius_given && !(std::isfinite(light_radius) && light_radius >= 0.0f))
	{
		std::cerr << "raytracer: --light-radius takes a finite radius >= 0" << std::endl;
		return SKR_ERR_ARG;
	}

	skr_scene *scene = nullptr;
	if(skr_scene_create_from_scn_ex(path, quiet ? 0 : 1, (strict_scn ? SKR_SCN_STRICT : 0u) | (scn_fog ? SKR_SCN_FOG : 0u) | (triangle_shadows ? SKR_SCN_TRIANGLE_SHADOWS : 0u) | (sphere_tree ? SKR_SCN_SPHERE_TREE : 0u) | (scn_spot ? SKR_SCN_SPOT : 0u) | (scn_motion ? SKR_SCN_MOTION : 0u) | (scn_texture ? SKR_SCN_TEXTURE : 0u) | (scn_emission ? SKR_SCN_EMISSION : 0u), &scene) != SKR_OK)
	{
		printf("%s\n", skr_last_error()); // scene.cpp:24-25: message, exit(0)
		return 0;
	}
	if(radius_given)
	{ // every point and spot light of the loaded scene (include/skr.h skr_scene_set_light_radii)
		int32_t n = 0;
		skr_scene_get_light_radii(scene, nullptr, &n);
		const std::vector<float> radii((size_t) n, light_radius);
		if(skr_scene_set_light_radii(scene, radii.data(), n) != SKR_OK)
		{
			std::cerr << "raytracer: " << skr_last_error() << std::endl;
			return SKR_ERR_ARG;
		}
	}
	if(aperture_given && skr_scene_set_lens(scene, aperture, focus) != SKR_OK)
	{ // (--focus without --aperture: accepted, no effect)
		std::cerr << "raytracer: --aperture takes a finite radius >= 0 and --focus a finite distance > 0" << std::endl;
		return SKR_ERR_ARG;
	}
	if(shutter_given && skr_scene_set_shutter(scene, shutter) != SKR_OK)
	{
		std::cerr << "raytracer: --shutter takes a finite number >= 0" << std::endl;
		return SKR_ERR_ARG;
	}
	if(envmap)
	{
		uint32_t ew = 0, eh = 0;
		if(skr_read_pfm(envmap, &ew, &eh, nullptr) != SKR_OK)
		{
			std::cerr << "raytracer: --envmap " << envmap << ": " << skr_last_error() << std::endl;
			return SKR_ERR_IO;
		}
		if(ew != eh || ew > (uint32_t) SKR_ENV_MAX_EDGE)
		{
			std::cerr << "raytracer: --envmap " << envmap << ": the environment must be square with an edge of at most " << SKR_ENV_MAX_EDGE << ", the file is " << ew << " x " << eh << std::endl;
			return SKR_ERR_ARG;
		}
		std::vector<float> tex((size_t) ew * eh * 3);
		if(skr_read_pfm(envmap, &ew, &eh, tex.data()) != SKR_OK || skr_scene_set_environment(scene, tex.data(), (int32_t) ew) != SKR_OK)
		{
			std::cerr << "raytracer: --envmap " << envmap << ": " << skr_last_error() << std::endl;
			return SKR_ERR_ARG;
		}
	}
	if(strict_scn)
	{ // the .scn's own film_resolution (scene.cpp:105-109) and max_depth (:192-198) hold unless the command line says otherwise
	  // (the reference parses both and then overrides / never reads them: main.cpp:393-395, scene.h:26)
		skr_scene_info info;
		skr_scene_get_info(scene, &info);
		if(!width_given && info.film_width > 0) option.width = info.film_width;
		if(!height_given && info.film_height > 0) option.height = info.film_height;
		if(!depth_given && info.max_depth_parsed > 0) option.max_depth = info.max_depth_parsed;
	}
	if(scn_fov && !fov_given)
	{ // camera.h:14 halfHeightAngle, parsed and never used by the reference: the .scn holds for what argv leaves open (2 h is exact)
		skr_scene_info info;
		skr_scene_get_info(scene, &info);
		option.fov = 2.0f * info.camera[12];
	}
	// utils.h:35-38 Options::to_string
	printf("\n\nMonte carlo: %d\nvisual display: %d\nfov: %f\nnum paths traced: %d\nsupersample grid size: %d\nmax depth: %d\n",
		   option.monte_carlo, visual ? 1 : 0, option.fov, option.num_path_traces, option.grid_size, option.max_depth);

	if(option.width <= 0 || option.height <= 0 || option.width > 65536 || option.height > 65536)
	{ // before anything is sized from it (the reference would allocate width x height vec3s here, main.cpp:125-128)
		std::cerr << "raytracer: bad image size " << option.width << "x" << option.height << std::endl;
		return SKR_ERR_ARG;
	}
	const bool want_pfm = !strcmp(format, "pfm"), want_png = !strcmp(format, "png");
	if(!want_pfm && !want_png && strcmp(format, "ppm"))
	{
		std::cerr << "format takes ppm, png or pfm" << std::endl;
		return 0;
	}
	if(sharded && (want_pfm || progressive_every))
	{ // the ranks exchange quantised tiles (one all-gather of bytes): the float frame and the running mean stay on their devices
		std::cerr << "raytracer: --format pfm and --progressive-every need the single-device path (drop --gpus)" << std::endl;
		return SKR_ERR_ARG;
	}
	if(denoised && ((sharded && gpus > 1) || progressive_every || denoise < 0 || denoise > SKR_DENOISE_MAX_ITERATIONS))
	{ // the filter needs whole-frame neighbours (the ranks exchange quantised tiles) and filters the finished mean only
		std::cerr << "raytracer: --denoise takes 0 .. " << SKR_DENOISE_MAX_ITERATIONS << " iterations on the single-device path (no --gpus N > 1, no --progressive-every)" << std::endl;
		return SKR_ERR_ARG;
	}
	if(adaptive && (option.progressive_passes > 1 || progressive_every || (sharded && gpus > 1) || denoised))
	{ // the passes are chosen per pixel on one device; --denoise estimates its variance spatially, --adaptive-denoise takes the measured one
		std::cerr << "raytracer: --adaptive cannot be combined with --progressive K > 1, --progressive-every, --gpus N > 1 or --denoise (--adaptive-denoise L filters an adaptive frame)" << std::endl;
		return SKR_ERR_ARG;
	}
	if(adaptive_denoised && (!adaptive || denoised || adaptive_denoise < 0 || adaptive_denoise > SKR_DENOISE_MAX_ITERATIONS))
	{
		std::cerr << "raytracer: --adaptive-denoise takes 0 .. " << SKR_DENOISE_MAX_ITERATIONS << " iterations, needs --adaptive T and excludes --denoise" << std::endl;
		return SKR_ERR_ARG;
	}
	if(denoised || adaptive) sharded = false; // (--gpus 1: the one device)
	std::vector<uint8_t> rgb((size_t) option.width * option.height * 3);
	std::vector<float> rgbf(want_pfm ? rgb.size() : 0);
	struct Out {
		const char *path;
		uint32_t w, h;
		bool pfm, png, quiet;
	} out{output, (uint32_t) option.width, (uint32_t) option.height, want_pfm, want_png, quiet};
	auto write_out = [](const Out &o, const uint8_t *b, const float *f) {
		return o.pfm ? skr_write_pfm(o.path, o.w, o.h, f) : o.png ? skr_write_png(o.path, o.w, o.h, b) : skr_write_ppm(o.path, o.w, o.h, b);
	};
	float ms = 0;
	uint64_t counters[3] = {0, 0, 0};
	int rc;
	skr_renderer *renderer = nullptr;
	skr_multi *multi = nullptr;
	if(sharded)
	{ // one process, N devices: interleaved row tiles, one RCCL all-gather, the root de-interleaves (include/skr.h "multi-GPU")
		rc = skr_multi_create(scene, gpus, nullptr, &multi);
		if(rc == SKR_OK) rc = skr_multi_render_frame_host(multi, &option, tile_rows, rgb.data(), &ms);
		if(rc != SKR_OK)
		{
			std::cerr << "raytracer: " << skr_last_error() << std::endl;
			return rc; // new failure class (the reference has no device): non-zero
		}
		for(int i = 0; i < gpus; i++)
		{
			uint64_t c[3] = {0, 0, 0};
			skr_renderer_read_counters(skr_multi_renderer(multi, i), c, 0);
			for(int k = 0; k < 3; k++) counters[k] += c[k];
		}
	}
	else
	{
		// --progressive-every: the file is the window (main.cpp:183-197 redraws its SDL window as rows finish) — rewritten with the
		// mean so far after every M passes
		struct Show {
			const Out *o;
			int (*write)(const Out &, const uint8_t *, const float *);
		} show{&out, write_out};
		skr_progress_fn progress = [](void *user, uint32_t done, uint32_t passes, const uint8_t *b, const float *f) -> int {
			const Show *s = static_cast<const Show *>(user);
			if(done < passes && s->write(*s->o, b, f) != SKR_OK) return 1;
			if(!s->o->quiet) printf("pass %u of %u\n", done, passes);
			return 0;
		};
		rc = skr_renderer_create(scene, device, &renderer);
		std::vector<uint32_t> passes(adaptive ? (size_t) option.width * option.height : 0);
		if(rc == SKR_OK && adaptive)
		{
			if(adaptive_denoised)
				rc = skr_render_adaptive_denoised_host(renderer, &option, &adapt, (uint32_t) adaptive_denoise, want_pfm ? nullptr : rgb.data(),
													   want_pfm ? rgbf.data() : nullptr, passes.data(), &ms);
			else rc = skr_render_adaptive_host(renderer, &option, &adapt, want_pfm ? nullptr : rgb.data(), want_pfm ? rgbf.data() : nullptr, passes.data(), &ms);
			if(rc == SKR_OK)
			{ // the mean passes per pixel and the share of pixels that reached max_passes
				uint64_t sum = 0, at_max = 0;
				for(uint32_t n : passes)
				{
					sum += n;
					at_max += n == (uint32_t) adapt.max_passes;
				}
				fprintf(stderr, "adaptive: %.3f passes per pixel (min %d, max %d, threshold %g), %.2f %% of the pixels at max\n", (double) sum / passes.size(),
						adapt.min_passes, adapt.max_passes, (double) adapt.threshold, 100.0 * (double) at_max / passes.size());
			}
		}
		else if(rc == SKR_OK && denoised)
			rc = skr_render_denoised_host(renderer, &option, (uint32_t) denoise, want_pfm ? nullptr : rgb.data(), want_pfm ? rgbf.data() : nullptr, &ms);
		else if(rc == SKR_OK)
			rc = skr_render_progressive_host(renderer, &option, progressive_every, want_pfm ? nullptr : rgb.data(), want_pfm ? rgbf.data() : nullptr,
											 progressive_every ? progress : nullptr, &show, &ms);
		if(rc != SKR_OK)
		{
			std::cerr << "raytracer: " << skr_last_error() << std::endl;
			return rc;
		}
		skr_renderer_read_counters(renderer, counters, 0);
	}
	rc = write_out(out, rgb.data(), rgbf.data());
	if(rc != SKR_OK)
	{
		std::cerr << "raytracer: " << skr_last_error() << std::endl;
		return rc;
	}
	printf("***\nWROTE TO PPM\n***\n"); // main.cpp:213
	fprintf(stderr, "{\"gpus\": %d, \"kernel\": \"%s\", \"frame_ms\": %.3f, \"radiance_rays\": %llu, \"mrays_per_s\": %.1f, \"shadow_rays\": %llu}\n",
			gpus > 1 ? gpus : 1, skr_kernel_variant(), ms, (unsigned long long) counters[0], ms > 0 ? counters[0] / (ms * 1e3) : 0.0, (unsigned long long) counters[2]);
	skr_multi_destroy(multi);
	skr_renderer_destroy(renderer);
	skr_scene_destroy(scene);
	return 0;
}
