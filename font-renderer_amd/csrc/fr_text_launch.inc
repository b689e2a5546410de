// fr_text_launch.inc — from a text plan's parameters to its kernel instance and that instance's name: the host half of
// launch_text (fr_text.hpp), included into the unnamed namespace of each translation unit that defines text kernels
// (fr_text.hip, fr_text_affine.hip).  The unit defines first: text_form<ARGS>() (the part of the name between "text_" and
// the family) and text_kernel_of<ARGS, FAM, FILL, BLEND, N>() (the instance).  After its unnamed namespace it states
// FR_TEXT_LAUNCH_FOR(ARGS) once per argument type it serves: launch_text's specialisation for it.
struct Launch {
    uint32_t n_tiles;
    hipStream_t stream;
    char *name;
    size_t name_cap;
};

template <class ARGS, int FAM, int FILL, int BLEND, int N>
hipError_t launch_instance(const ARGS &a, const Launch &l)
{
    constexpr const char *family[5] = {"", "rgba_", "srgb_", "rgba_load_", "srgb_load_"};
    void (*kernel)(ARGS) = text_kernel_of<ARGS, FAM, FILL, BLEND, N>();
    if (l.name) {                                                          // as rocprofv3 names the instance
        if constexpr (FAM == 0) snprintf(l.name, l.name_cap, "fr::text_%skernel<%d, %d>", text_form<ARGS>(), N, FILL);
        else snprintf(l.name, l.name_cap, "fr::text_%s%skernel<%d, %d, %d>", text_form<ARGS>(), family[FAM], N, FILL, BLEND);
    }
    if (!l.n_tiles) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(l.n_tiles), dim3(64 * TEXT_WAVES), 0, l.stream, a);
    return hipGetLastError();
}

template <class ARGS, int FAM, int FILL, int BLEND>
hipError_t launch_n(const ARGS &a, int n, const Launch &l)
{
    if (n == 4) return launch_instance<ARGS, FAM, FILL, BLEND, 4>(a, l);
    if (n == 2) return launch_instance<ARGS, FAM, FILL, BLEND, 2>(a, l);
    return launch_instance<ARGS, FAM, FILL, BLEND, 1>(a, l);
}

template <class ARGS, int FAM>
hipError_t launch_family(const ARGS &a, int n, int fill, int blend, const Launch &l)
{
    if constexpr (FAM != 0) {                                              // (the coverage kernels have no BLEND)
        if (blend == 2) return fill ? launch_n<ARGS, FAM, 1, 2>(a, n, l) : launch_n<ARGS, FAM, 0, 2>(a, n, l);
    }
    if (blend) return fill ? launch_n<ARGS, FAM, 1, 1>(a, n, l) : launch_n<ARGS, FAM, 0, 1>(a, n, l);
    return fill ? launch_n<ARGS, FAM, 1, 0>(a, n, l) : launch_n<ARGS, FAM, 0, 0>(a, n, l);
}

template <class ARGS>
hipError_t launch_any(const ARGS &a, int n, int fill, int rgba, int blend, int srgb, int load, const Launch &l)
{
    if (!rgba) return launch_family<ARGS, 0>(a, n, fill, 0, l);
    if (load) return srgb ? launch_family<ARGS, 4>(a, n, fill, blend, l) : launch_family<ARGS, 3>(a, n, fill, blend, l);
    return srgb ? launch_family<ARGS, 2>(a, n, fill, blend, l) : launch_family<ARGS, 1>(a, n, fill, blend, l);
}

#define FR_TEXT_LAUNCH_FOR(ARGS)                                                                                            \
    template <>                                                                                                             \
    hipError_t launch_text(const ARGS &a, int n, int fill, int rgba, int blend, int srgb, int load, uint32_t n_tiles,      \
                           hipStream_t stream, char *name, size_t name_cap)                                                 \
    {                                                                                                                       \
        return launch_any(a, n, fill, rgba, blend, srgb, load, Launch{n_tiles, stream, name, name_cap});                    \
    }
