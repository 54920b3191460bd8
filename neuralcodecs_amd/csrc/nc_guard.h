// The C-ABI wrappers' side of a handle (nc_api.hip, nc_chunk.hip): exception -> status translation and the checked way from the
// opaque nc_codec to the engine object behind it.
#pragma once
#include <new>

#include "nc_model.h"

namespace nc {

template <class F>
nc_status guard(F&& f) {
    try {
        f();
        return NC_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return NC_ENOMEM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return NC_ESTATE;
    }
}

inline Codec& codec_of(const nc_codec* h) {
    if (!h || !h->impl) fail(NC_EINVAL, "null codec handle");
    return *h->impl;
}

// the model of kind M::kKind behind the handle (query entry points take the handle const: the object itself is not)
template <class M>
M& as(const nc_codec* h) {
    Codec& c = codec_of(h);
    if (h->kind != M::kKind) fail(NC_EINVAL, "handle is not %s codec", M::kKindName);
    return static_cast<M&>(c);
}

}  // namespace nc
