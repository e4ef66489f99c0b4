#pragma once
// Shared by the capi_*.cpp files: the extern "C" layer of libsealhip.so — see include/sealhip.h.  Every body is closed by the same
// exception-to-HRESULT ladder as the reference's C export layer (SEAL_C_CATCH_ALL,
// native/src/seal/c/defines.h:75-97); null handles return E_POINTER like IfNullRet
// (native/src/seal/c/utilities.h).
#include "../../include/sealhip.h"
#include "evaluator.h"
#include "ckks_encoder.h"
#include "decryptor.h"
#include "keygen.h"
#include "serial.h"
#include "xof.h"
#include <atomic>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <type_traits>

namespace sealhip
{
    // message of the calling thread's last failed call (SealHip_LastError); one instance for all capi_*.cpp files (capi_core.cpp)
    std::string &capi_last_error();
    // SEALContext_Destroy: the ContextData handles given out for this context die with it (capi_containers.cpp)
    void capi_forget_context(const class Context *context);
}
using namespace sealhip;

namespace
{

    struct EncParams
    {
        uint8_t scheme = 0;
        uint64_t n = 0;
        std::vector<uint64_t> coeff_modulus;
        uint64_t plain_modulus = 0;
    };
    struct Timer
    {
        hipEvent_t e0 = nullptr, e1 = nullptr;
    };

#define SHL_TRY \
    try         \
    {
#define SHL_CATCH                               \
    }                                           \
    catch (const std::invalid_argument &e)      \
    {                                           \
        sealhip::capi_last_error() = e.what();                \
        return SHL_E_INVALIDARG;                \
    }                                           \
    catch (const std::out_of_range &e)          \
    {                                           \
        sealhip::capi_last_error() = e.what();                \
        return SHL_E_INVALID_INDEX;             \
    }                                           \
    catch (const std::logic_error &e)           \
    {                                           \
        sealhip::capi_last_error() = e.what();                \
        return SHL_COR_E_INVALIDOPERATION;      \
    }                                           \
    catch (const std::runtime_error &e)         \
    {                                           \
        sealhip::capi_last_error() = e.what();                \
        return SHL_COR_E_IO;                    \
    }                                           \
    catch (const std::bad_alloc &)              \
    {                                           \
        sealhip::capi_last_error() = "out of device memory";  \
        return SHL_E_OUTOFMEMORY;               \
    }                                           \
    catch (...)                                 \
    {                                           \
        sealhip::capi_last_error() = "unexpected exception";  \
        return SHL_E_UNEXPECTED;                \
    }                                           \
    return SHL_S_OK;

#define IfNullRet(p, r) \
    if (!(p))           \
    return (r)

    template <typename T>
    T *as(void *p)
    {
        return static_cast<T *>(p);
    }

    void hip_ok(hipError_t e, const char *what)
    {
        if (e != hipSuccess)
            throw std::runtime_error(std::string("HIP failure in ") + what + ": " + hipGetErrorString(e));
    }

    // dest = src unless they are the same object (the sealc "destination" convention)
    Ciphertext &prepare_dest(void *encrypted, void *destination)
    {
        Ciphertext *src = as<Ciphertext>(encrypted), *dst = as<Ciphertext>(destination);
        if (src != dst)
            *dst = *src;
        return *dst;
    }

    // The body of every entry: E_POINTER when one of `handles` is null - the pointers an entry dereferences itself; a pointer that
    // is optional or that the C++ layer refuses (std::invalid_argument) is not listed.  Then body() runs inside the exception
    // ladder; it returns nothing (S_OK) or an SHL_HRESULT of its own.  A template, so outside every extern "C" block.
    template <class Body>
    SHL_HRESULT guarded(std::initializer_list<const void *> handles, Body body)
    {
        for (const void *handle : handles)
            IfNullRet(handle, SHL_E_POINTER);
        SHL_TRY
        if constexpr (std::is_void<decltype(body())>::value)
            body();
        else
            return body();
        SHL_CATCH
    }

    // The body of an Evaluator_* operation (capi_evaluator.cpp): guarded, thisptr first, and body(evaluator) under a StreamScope on
    // the evaluator's stream: the one scope an operation needs, whichever thread calls (evaluator.h: Evaluator::stream_).
    template <class Body>
    SHL_HRESULT ev_call(void *thisptr, std::initializer_list<const void *> handles, Body body)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        return guarded(handles, [&] {
            Evaluator &ev = *as<Evaluator>(thisptr);
            StreamScope stream_scope(ev.stream());
            body(ev);
        });
    }

    static const uint64_t kParmsIdZero[4] = { 0, 0, 0, 0 };
    // a parms_id getter: the level's, parms_id_zero without one
    inline void copy_parms_id(uint64_t *parms_id, const Level *level)
    {
        std::memcpy(parms_id, level ? level->parms_id : kParmsIdZero, 32);
    }

    // ---- the object streams (serial.h).  A serialisable object supplies raw_bytes() - the size of its uncompressed stream - and
    // write(dst, capacity), which lays the stream down (serial::Writer or a serial::save_* refuses a short dst) and copies its
    // words from the device.  *_SaveSize and *_Save are these two, inside guarded.
    template <class RawBytes>
    void save_size(uint8_t compr_mode, int64_t *result, RawBytes raw_bytes)
    {
        if (!serial::compr_mode_supported(compr_mode))
            throw std::invalid_argument("unsupported compression mode");
        *result = (int64_t)serial::compress_bound(raw_bytes(), compr_mode);
    }
    // uncompressed: straight into the caller's buffer, whose capacity write() checks; compressed: through a host image of the raw
    // stream, and serial::compress_stream checks the capacity
    template <class RawBytes, class Write>
    void save_stream(uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes, RawBytes raw_bytes, Write write)
    {
        if (!serial::compr_mode_supported(compr_mode))
            throw std::invalid_argument("unsupported compression mode");
        const size_t bytes = raw_bytes();
        if (compr_mode == 0)
        {
            write(outptr, (size_t)size);
            *out_bytes = (int64_t)bytes;
            return;
        }
        std::vector<uint8_t> raw(bytes);
        write(raw.data(), bytes);
        *out_bytes = (int64_t)serial::compress_stream(raw.data(), bytes, compr_mode, outptr, (size_t)size);
    }
    // *_Load / *_UnsafeLoad of an object that takes a context: parse(object, context) returns the bytes read
    template <class Object, class Parse>
    SHL_HRESULT load_stream(void *thisptr, void *context, uint8_t *inptr, int64_t *in_bytes, Parse parse)
    {
        return guarded({ thisptr, context, inptr, in_bytes }, [&] { *in_bytes = (int64_t)parse(*as<Object>(thisptr), *as<Context>(context)); });
    }
    // the seeded piece of an image whose words go to `dst` (serial.h: pending_words after the stored ones), as the device's job (xof.h)
    inline XofJob seeded_piece(const serial::CiphertextImage &img, uint64_t *dst)
    {
        XofJob job;
        std::memcpy(job.seed, img.pending_seed, sizeof(job.seed));
        job.prng_type = img.pending_type;
        job.dst = dst + img.stored_words;
        return job;
    }
} // namespace
