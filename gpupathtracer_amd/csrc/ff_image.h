// ff_image.h — what the image-space entry points (ff_image_api.cpp: ff_gbuffer, ff_denoise, ff_denoise_temporal, ff_taa;
// ff_display_api.cpp; ff_upscale_api.cpp; the filters of the ff_*_api.cpp files behind them) keep in the tracer state and share:
// the staging of host buffers through the state's one image work buffer, the size and overlap checks, and the reprojection
// history.  Nothing here reaches a trace kernel.
#pragma once

#include <initializer_list>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_internal.h"

namespace ff {

struct TemporalGeom; // ff_temporal.h

// Host buffers travel through a device buffer the state owns (FfState::d_img_work for every image-space entry point; the bytes
// before `first_byte` are the entry point's own scratch), in 16-byte aligned pieces from `first_byte` on.  The caller names
// its pieces once - in(): copied to the device by commit(), out(): copied back by finish() - so the size of the buffer and every
// piece's place in it come from the same list.  commit() grows the buffer, stores each piece's device address through the pointer
// it was registered with and enqueues the copies in; finish() runs after the caller's synchronize.
struct Staging {
    Staging(void** buffer, size_t* capacity, size_t first_byte = 0) : buf(buffer), cap(capacity), used(first_byte) {}
    template <class T>
    void in(const T** dev, const void* src, size_t bytes, hipMemcpyKind kind = hipMemcpyHostToDevice) { add((void**)dev, src, nullptr, bytes, kind); }
    template <class T>
    void out(T** dev, void* host, size_t bytes) { add((void**)dev, nullptr, host, bytes, hipMemcpyDeviceToHost); }
    int commit(hipStream_t stream, const char* copy_failed); // copy_failed: the error text of a failed copy in (null: the HIP call's)
    int finish();

private:
    struct Piece {
        void** dev;
        const void* src;
        void* host;
        size_t offset, bytes;
        hipMemcpyKind kind;
    };
    void add(void** dev, const void* src, void* host, size_t bytes, hipMemcpyKind kind)
    {
        pieces.push_back({ dev, src, host, used, bytes, kind });
        used += (bytes + 15) & ~(size_t)15;
    }
    void** buf;
    size_t* cap;
    size_t used;
    std::vector<Piece> pieces;
};

// The two optional outputs of an image filter of `px` output pixels, as the kernel gets them: the caller's device pointers, or
// pieces of `stage` that finish() copies back to the caller's host buffers.  Null stays null.  (Not copyable: commit() stores the
// pieces' addresses through the two members.)
struct StagedOutputs {
    unsigned char* rgb8;
    float* radiance;
    StagedOutputs(Staging& stage, size_t px, void* rgb8_out, int rgb8_on_device, float* radiance_out, int radiance_out_on_device)
        : rgb8((unsigned char*)rgb8_out), radiance(radiance_out)
    {
        if (rgb8_out && !rgb8_on_device) stage.out(&rgb8, rgb8_out, px * 3);
        if (radiance_out && !radiance_out_on_device) stage.out(&radiance, radiance_out, px * 12);
    }
    StagedOutputs(const StagedOutputs&) = delete;
    StagedOutputs& operator=(const StagedOutputs&) = delete;
};

// What the filters refuse before they look at a buffer: an image size out of range ...
inline int check_image_size(int width, int height, const char* who)
{
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return fail(FF_ERR_INVALID_ARG, "%s: image size %dx%d is invalid", who, width, height);
    return FF_OK;
}

// ... and, as a gather reads neighbours, an output (rgb8, radiance_out; either may be null) that lies on an input or on the other
// output, which different lanes write.
struct Span {
    const void* ptr;
    size_t bytes;
    const char* name;
};

inline bool overlaps(const Span& a, const Span& b)
{
    const char* p = (const char*)a.ptr;
    const char* q = (const char*)b.ptr;
    return p < q + b.bytes && q < p + a.bytes;
}

inline int check_disjoint(const Span (&outs)[2], std::initializer_list<Span> ins, const char* who)
{
    for (const Span& o : outs)
        for (const Span& i : ins)
            if (o.ptr && overlaps(o, i)) return fail(FF_ERR_INVALID_ARG, "%s: %s overlaps %s", who, o.name, i.name);
    if (outs[0].ptr && outs[1].ptr && overlaps(outs[0], outs[1])) return fail(FF_ERR_INVALID_ARG, "%s: %s overlaps %s", who, outs[0].name, outs[1].name);
    return FF_OK;
}

// ... for the usual pair of outputs: rgb8 and radiance_out of `px` pixels.
inline int check_outputs_disjoint(const void* rgb8, const float* radiance_out, size_t px, std::initializer_list<Span> ins, const char* who)
{
    const Span outs[2] = { { rgb8, px * 3, "rgb8" }, { radiance_out, px * 12, "radiance_out" } };
    return check_disjoint(outs, ins, who);
}

// What the reprojecting filters and ff_interpolate prepare on the host (ff_image_api.cpp): the inverse of a 4x4 matrix in double
// (column-major in and out; false if singular), and inverse(ff_camera_ray_matrix(c)) rounded to float, with the ray matrix itself.
bool invert4(const double* m, double* out);
bool inverse_ray_matrix(const FfCamera* c, float* out16, FfMat4* ray);

// What a filter that reprojects its last result (ff_denoise_temporal, ff_taa) remembers between calls: two history sets in
// d_work that swap by index (`cur`: the one the last call wrote; the layout is the filter's own), and the camera, image size and
// per-geometry model matrices (caller's order) of that call.  `replaced` marks the meshes ff_update_mesh changed since.
struct ReprojectionHistory {
    float4* d_work = nullptr;
    size_t work_bytes = 0;
    void* d_geoms = nullptr; // the per-geometry table (TemporalGeom rows)
    size_t geoms_bytes = 0;
    std::vector<unsigned char> h_geoms; // its host copy (kept alive until the upload has completed)
    bool valid = false;                 // history to reproject from
    bool last = false;                  // a call's motion and lengths are there to read (ff_temporal_history / ff_taa_history)
    int cur = 0, width = 0, height = 0;
    FfCamera camera = {};
    std::vector<float> model; // 12 floats (model matrix columns, xyz) per caller geometry index
    std::vector<unsigned char> has_model, replaced;

    // One call of the filter: whether it reprojects, the set it writes, and the table (num rows on the device).
    struct Frame {
        bool has_history;
        int cur, num;
        const TemporalGeom* geoms;
    };
    // begin: the history is kept only for the same image size.  It is invalid from here until commit(), so a call that fails in
    // between leaves none; sizes d_work, builds the table from the previous call's model matrices and uploads it on `stream`.
    int begin(const std::vector<GeomRecord>& records, int w, int h, size_t work_bytes_needed, hipStream_t stream, Frame* out);
    // commit: the history now describes this call.
    void commit(const std::vector<GeomRecord>& records, const FfCamera* cam, int w, int h, const Frame& f);
    void invalidate() { valid = last = false; }
    void mark_replaced(int index)
    {
        if ((size_t)index < replaced.size()) replaced[index] = 1;
    }
    void release(); // frees the device buffers (ff_destroy)
};

} // namespace ff
