# Numeric and device compile flags of the MI355X-native library, shared with the programs that
# must compute exactly as it does (tests/cpp/device_units.hip).
# Numerics flags are part of the parity contract (sp_math.h): no FP contraction, IEEE div/sqrt,
# fp32 denormals preserved on the device.
NUMFLAGS := -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero -fhip-fp32-correctly-rounded-divide-sqrt
# Device code: no SLP vectorisation.  It packs independent f32 ops into v_pk_* instructions whose
# constant operand pairs get hoisted into VGPR pairs -- and, under the shading kernels' register
# pressure, spilled to scratch and reloaded inside the hot loops (wf_shade: 168 -> 64 B/lane of
# scratch without it, wf_primary 72 -> 57 VGPRs; same IEEE operations either way).
HIPFLAGS := -fno-slp-vectorize
