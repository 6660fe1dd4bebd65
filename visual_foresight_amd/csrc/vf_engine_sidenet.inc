// vf_engine_sidenet.inc - host plumbing the small networks beside the predictor share (vf_engine_scorer.inc,
// vf_engine_regnet.inc): device buffers, uploads, the weight packer and the launch of vf_net_conv.h.  Included at the end of
// vf_engine.hip, before them.  Under -DVF_HOST_SELFTEST allocations are address reservations and uploads are dropped, so
// the tensor tables, the packer and every refusal run under the sanitizers without a GPU.

namespace vf {

template <typename T>
static int side_alloc(std::vector<AllocRec> &allocs, T **p, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void *q = nullptr;
#ifdef VF_HOST_SELFTEST
    q = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);       // never dereferenced
    if (q == MAP_FAILED) return fail(VF_ERR_NOMEM, "self-test address reservation failed");
#else
    if (hipMalloc(&q, bytes) != hipSuccess)
        return fail(VF_ERR_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
#endif
    allocs.push_back({q, bytes});
    *p = reinterpret_cast<T *>(q);
    return VF_OK;
}

// net->ptr = n elements; a failure destroys the half-built net and leaves the create function (which declares `rc`)
#define VF_SIDE_ALLOC(net, destroy, ptr, n)                         \
    do {                                                            \
        rc = side_alloc((net)->allocs, &(ptr), (size_t)(n));        \
        if (rc) { destroy(net); return rc; }                        \
    } while (0)

static void side_free_all(int device, std::vector<AllocRec> &allocs) {
#ifdef VF_HOST_SELFTEST
    (void)device;
    for (const AllocRec &a : allocs) munmap(a.p, a.bytes);
#else
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    for (const AllocRec &a : allocs) (void)hipFree(a.p);
#endif
}

static int side_upload(void *dst, const void *src, size_t bytes) {
#ifdef VF_HOST_SELFTEST
    (void)dst; (void)src; (void)bytes;
#else
    VF_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
#endif
    return VF_OK;
}

static size_t packed_floats(int Cin, int Cout) { return (size_t)9 * Cin * ((Cout + 31) / 32) * 32; }

// canonical [3][3][Cin][Cout] -> [step][half][ceil(Cout / 32)][32][4] (vf_net_conv.h): step = tap * Cin / 8 + block; the
// columns past Cout stay zero
static void pack_conv3x3_mfma(const float *w, int Cin, int Cout, std::vector<float> &out) {
    const int blocks = Cin / 8, ntile = (Cout + 31) / 32;
    out.assign(packed_floats(Cin, Cout), 0.f);
    for (int tap = 0; tap < 9; ++tap)
        for (int blk = 0; blk < blocks; ++blk)
            for (int half = 0; half < 2; ++half)
                for (int nt = 0; nt < ntile; ++nt)
                    for (int j = 0; j < 32 && 32 * nt + j < Cout; ++j)
                        for (int q = 0; q < 4; ++q) {
                            const size_t step = (size_t)tap * blocks + blk;
                            const size_t dst = ((((step * 2 + half) * ntile + nt) * 32 + j) * 4) + q;
                            const size_t src = ((size_t)tap * Cin + 8 * blk + 4 * half + q) * Cout + 32 * nt + j;
                            out.at(dst) = w[src];
                        }
}

// Walks one view's part of a canonical weight blob, tensor by tensor, into the per-view device arrays.  After the first
// failed upload nothing more is copied; `rc` keeps that error.
struct BlobCursor {
    const float *p;             // the next tensor of the view's blob
    int view;
    int rc = VF_OK;
    std::vector<float> packed;

    // the next n floats as they are -> dst_base + view * n
    void upload(float *dst_base, size_t n) {
        if (rc) return;
        rc = side_upload(dst_base + view * n, p, n * sizeof(float));
        p += n;
    }
    // the next [3][3][Cin][Cout] packed for vf_net_conv.h -> dst_base + view * packed_floats(Cin, Cout)
    void upload_packed(float *dst_base, int Cin, int Cout) {
        if (rc) return;
        pack_conv3x3_mfma(p, Cin, Cout, packed);
        rc = side_upload(dst_base + view * packed.size(), packed.data(), packed.size() * sizeof(float));
        p += (size_t)9 * Cin * Cout;
    }
};

#ifndef VF_HOST_SELFTEST
// one wave per (image, position tile, channel group) task, kNetConvThreads / 64 of them per workgroup (net_conv_task)
template <typename... KA, typename... A>
static void launch_net_conv(void (*kernel)(KA...), long long n_img, long long mtiles, int ngroups, hipStream_t st, A... args) {
    const long long tasks = n_img * mtiles * ngroups;
    constexpr int per_block = kNetConvThreads / 64;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((tasks + per_block - 1) / per_block)), dim3(kNetConvThreads), 0, st, args...);
}
#endif

}  // namespace vf
