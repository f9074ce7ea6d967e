--[[ Materials whose programs declare more registers than the GPU interpreter's in-register file (16 numbers, 8 vectors,
     8 RGBs): both front ends give every value a register of its own, and pyr_scene_create renumbers them. ]]
local blend = rgb(0.9, 0.2, 0.1) * 0.3 + rgb(0.1, 0.8, 0.1) * 0.3 + rgb(0.1, 0.1, 0.9) * 0.4

local nested = mix(mix(mix(mix(mix(mix(material.diffuse {color = 0.8}, material.mirror {color = 0.8}, fresnel(1.3)),
    material.mirror {color = 0.7}, fresnel(1.4)), material.mirror {color = 0.6}, fresnel(1.5)), material.mirror {color = 0.5},
    fresnel(1.6)), material.mirror {color = 0.4}, fresnel(1.7)),
    material.mirror {color = 0.3}, fresnel(1.8))

local bumps = texture("../textures/tiles_normal.png", "linear") * vector(1, -1, 1) + vector(0.1, 0, 0)
bumps = (bumps * vector(0.9, 1, 1) + vector(0, 0.05, 0)) * vector(1, 0.95, 1) + vector(0, 0, 0.1)

return {
    image = {width = 48, height = 32},

    renderer = renderer.simple {pixel_samples = 4, spectrum_samples = 6, tile_size = 16, bounces = 4, light_samples = 1},

    camera = camera.perspective {
        fov = 50,
        transform = transform.look_at {from = vector(0, 2, 8), to = vector(0, 1, 0)},
    },

    world = {
        sky = light_source.d65 * 0.2,
        objects = {
            shape.plane {
                origin = vector(), normal = vector {y = 1}, texture_scale = 4,
                material = {surface = material.diffuse {color = 0.6}, normal_map = bumps},
            },
            shape.sphere {radius = 0.8, position = vector(-1.8, 0.8, 0), material = {surface = material.diffuse {color = blend}}},
            shape.sphere {radius = 0.8, position = vector(0, 0.8, 0), material = {surface = nested}},
            shape.sphere {radius = 0.5, position = vector(1.8, 0.5, 0), material = {surface = material.emissive {color = light_source.d65 * 2}}},
        },
    },
}
