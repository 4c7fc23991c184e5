// One more function of bevy_core_pipeline 0.9.1's src/tonemapping/tonemapping_shared.wgsl, restated from the published source like
// the rest of bevy_0_9_1.wgsl: overlay.wgsl's inverse_reintard_luminance calls it.  Kept in a file of its own and appended to the
// `bevy_core_pipeline::tonemapping` module by the one test that executes overlay.wgsl (tests/test_present.py).

#define_import_path bevy_core_pipeline::tonemapping

fn tonemapping_change_luminance(c_in: vec3<f32>, l_out: f32) -> vec3<f32> {
    let l_in = tonemapping_luminance(c_in);
    return c_in * (l_out / l_in);
}
