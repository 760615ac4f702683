// Arithmetic that both halves of the library compile from the same source: the host's scene conversion (pt_convert.cpp, a plain C++ unit) and the
// kernels (ptamd.hip).  So a node the host packs and one the device re-packs after a refit or for a world-space copy hold the same bytes.  No kernels and
// no device-only intrinsics here.
#pragma once
#include "pt_device.h"
#include <cmath>

namespace ptd {

struct V3 {
    float x, y, z;
};
__host__ __device__ inline V3 mk(float x, float y, float z) { return { x, y, z }; }
__host__ __device__ inline V3 mk(float s) { return { s, s, s }; }
__host__ __device__ inline V3 xyz(float4 f) { return { f.x, f.y, f.z }; }
__host__ __device__ inline V3 operator+(V3 a, V3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
__host__ __device__ inline V3 operator-(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
__host__ __device__ inline V3 operator-(V3 a) { return { -a.x, -a.y, -a.z }; }
__host__ __device__ inline V3 operator*(V3 a, V3 b) { return { a.x * b.x, a.y * b.y, a.z * b.z }; }
__host__ __device__ inline V3 operator*(V3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }
__host__ __device__ inline V3 operator*(float s, V3 a) { return { s * a.x, s * a.y, s * a.z }; }
__host__ __device__ inline V3 operator/(V3 a, float s) { return { a.x / s, a.y / s, a.z / s }; }
__host__ __device__ inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ inline V3 cross(V3 a, V3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__host__ __device__ inline V3 normalize(V3 a)
{
    float len = sqrtf(dot(a, a));
    return { a.x / len, a.y / len, a.z / len };
}

// Quantise up to four child boxes into a WideNode (pt_device.h): origin = min corner of their union, per-axis power-of-two scale
// with (extent / scale) <= 255, planes rounded OUTWARDS and then verified with the exact expression the traversal kernels evaluate
// (origin + scale * q).  An empty slot gets an inverted box and `emptyRef`.  Shared by the host (collapse of the caller's binary
// trees) and the device (world-space copies), so that both produce the same bytes from the same boxes.
__host__ __device__ inline void quantiseWideNode(const float (*lo)[3], const float (*hi)[3], const uint32_t* refs, const bool* empty, uint32_t emptyRef, WideNode* out)
{
    float nlo[3] = { 3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f }, nhi[3] = { -3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f };
    for (int k = 0; k < 4; k++)
        for (int a = 0; a < 3; a++)
            if (!empty[k] && lo[k][a] <= hi[k][a]) {
                nlo[a] = fminf(nlo[a], lo[k][a]);
                nhi[a] = fmaxf(nhi[a], hi[k][a]);
            }
    WideNode w {};
    float scale[3];
    for (int a = 0; a < 3; a++) {
        if (!(nlo[a] <= nhi[a]))
            nlo[a] = nhi[a] = 0.f;
        // smallest power of two s with (hi - lo) / s <= 255, evaluated in float like the kernel does
        int e = 0;
        const float extent = nhi[a] - nlo[a];
        (void)frexpf(extent / 255.0f, &e); // extent/255 = m * 2^e, m in [0.5,1)  =>  2^e >= extent/255
        e = e < -126 ? -126 : (e > 127 ? 127 : e);
        scale[a] = ldexpf(1.0f, e);
        while (extent > 0.f && nlo[a] + scale[a] * 255.0f < nhi[a] && e < 127) // guard float round-off
            scale[a] = ldexpf(1.0f, ++e);
    }
    w.ox = nlo[0], w.oy = nlo[1], w.oz = nlo[2];
    w.scaleX = scale[0], w.scaleY = scale[1], w.scaleZ = scale[2];
    uint32_t q[6] = { 0, 0, 0, 0, 0, 0 }; // qlox, qhix, qloy, qhiy, qloz, qhiz
    for (int k = 0; k < 4; k++) {
        w.child[k] = empty[k] ? emptyRef : refs[k];
        for (int a = 0; a < 3; a++) {
            uint32_t ql = 255, qh = 0;
            if (!empty[k]) {
                const float fl = floorf((lo[k][a] - nlo[a]) / scale[a]);
                const float fh = ceilf((hi[k][a] - nlo[a]) / scale[a]);
                ql = (uint32_t)fmaxf(0.f, fminf(255.f, fl));
                qh = (uint32_t)fmaxf(0.f, fminf(255.f, fh));
                while (ql > 0 && nlo[a] + scale[a] * (float)ql > lo[k][a])
                    ql--;
                while (qh < 255 && nlo[a] + scale[a] * (float)qh < hi[k][a])
                    qh++;
            }
            q[a * 2] |= ql << (8 * k);
            q[a * 2 + 1] |= qh << (8 * k);
        }
    }
    w.qlox = q[0], w.qhix = q[1], w.qloy = q[2], w.qhiy = q[3], w.qloz = q[4], w.qhiz = q[5];
    *out = w;
}

} // namespace ptd
