// extern "C" layer, part 3: KSwitchKeys, Evaluator (ciphertext, plaintext-operand and many-operand forms), communicator and digit-parallel forms (include/sealhip.h)
#include "capi_common.h"
#include "batch_reduce_kernels.h"

namespace
{
    // what a handle is (checked by ev_call before a body runs)
    Ciphertext &ct(void *p)
    {
        return *as<Ciphertext>(p);
    }
    Plaintext &pt(void *p)
    {
        return *as<Plaintext>(p);
    }
    KSwitchKeys &keys(void *p)
    {
        return *as<KSwitchKeys>(p);
    }
    Plaintext &prepare_plain_dest(void *plain, void *destination)
    {
        Plaintext *src = as<Plaintext>(plain), *dst = as<Plaintext>(destination);
        if (src != dst)
            *dst = *src;
        return *dst;
    }
    std::vector<const Ciphertext *> ct_list(uint64_t count, void **encrypteds)
    {
        std::vector<const Ciphertext *> v;
        for (uint64_t i = 0; i < count; i++)
            v.push_back(as<Ciphertext>(encrypteds[i]));
        return v;
    }
    void check_flags(uint64_t flags, uint64_t defined)
    {
        if (flags & ~defined)
            throw std::invalid_argument("unknown flags");
    }
    Evaluator::KsExchange exchange_of(int how)
    {
        if (how != 0 && how != 1)
            throw std::invalid_argument("exchange: 0 = all-reduce, 1 = reduce-scatter + all-gather");
        return how ? Evaluator::KsExchange::reduce_scatter : Evaluator::KsExchange::all_reduce;
    }
} // namespace

extern "C"
{
    // ------------------------------------------------------------------ KSwitchKeys
    SHL_FUNC KSwitchKeys_Create1(void **kswitch_keys)
    {
        IfNullRet(kswitch_keys, SHL_E_POINTER);
        SHL_TRY
        *kswitch_keys = new KSwitchKeys();
        SHL_CATCH
    }
    SHL_FUNC KSwitchKeys_Destroy(void *thisptr)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        delete as<KSwitchKeys>(thisptr);
        return SHL_S_OK;
    }
    SHL_FUNC KSwitchKeys_Size(void *thisptr, uint64_t *size)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        IfNullRet(size, SHL_E_POINTER);
        *size = as<KSwitchKeys>(thisptr)->size();
        return SHL_S_OK;
    }
    SHL_FUNC KSwitchKeys_SetKey(void *thisptr, void *context, uint64_t index, uint64_t digits, const uint64_t *host_words)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(host_words, SHL_E_POINTER);
        SHL_TRY
        as<KSwitchKeys>(thisptr)->set_key(*as<Context>(context), index, digits, host_words, false);
        SHL_CATCH
    }
    SHL_FUNC KSwitchKeys_SetKeyFromDevice(void *thisptr, void *context, uint64_t index, uint64_t digits, const uint64_t *device_words)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(device_words, SHL_E_POINTER);
        SHL_TRY
        as<KSwitchKeys>(thisptr)->set_key(*as<Context>(context), index, digits, device_words, true);
        SHL_CATCH
    }
    SHL_FUNC KSwitchKeys_SetKeyDigits(void *thisptr, void *context, uint64_t index, uint64_t digit_first, uint64_t digits,
                                      const uint64_t *host_words)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(host_words, SHL_E_POINTER);
        SHL_TRY
        as<KSwitchKeys>(thisptr)->set_key(*as<Context>(context), index, digits, host_words, false, digit_first);
        SHL_CATCH
    }
    SHL_FUNC KSwitchKeys_HasKey(void *thisptr, uint64_t index, bool *has_key)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        IfNullRet(has_key, SHL_E_POINTER);
        *has_key = as<KSwitchKeys>(thisptr)->has_key(index);
        return SHL_S_OK;
    }
    SHL_FUNC RelinKeys_GetIndex(uint64_t key_power, uint64_t *index)
    {
        IfNullRet(index, SHL_E_POINTER);
        SHL_TRY
        *index = Evaluator::relin_index(key_power);
        SHL_CATCH
    }
    SHL_FUNC GaloisKeys_GetIndex(uint32_t galois_elt, uint64_t *index)
    {
        IfNullRet(index, SHL_E_POINTER);
        SHL_TRY
        *index = Evaluator::galois_index(galois_elt);
        SHL_CATCH
    }
    SHL_FUNC GaloisTool_GetEltFromStep(void *context, int step, uint32_t *galois_elt)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(galois_elt, SHL_E_POINTER);
        SHL_TRY
        Evaluator ev(*as<Context>(context));
        *galois_elt = ev.galois_elt_from_step(step);
        SHL_CATCH
    }

    // ------------------------------------------------------------------ Evaluator
    // Lifetime, stream and recording are not operations: they run outside ev_call's scope (set_stream and the recording change the
    // stream that scope would be on).  Every operation below is one ev_call: the handles whose NULL is E_POINTER, and the call.
    SHL_FUNC Evaluator_Create(void *context, void **evaluator)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(evaluator, SHL_E_POINTER);
        SHL_TRY
        *evaluator = new Evaluator(*as<Context>(context));
        SHL_CATCH
    }
    SHL_FUNC Evaluator_Destroy(void *thisptr)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        delete as<Evaluator>(thisptr);
        return SHL_S_OK;
    }
    SHL_FUNC Evaluator_SetStream(void *thisptr, void *hip_stream)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        SHL_TRY
        as<Evaluator>(thisptr)->set_stream((hipStream_t)hip_stream);
        SHL_CATCH
    }
    SHL_FUNC Evaluator_BeginCapture(void *thisptr)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        SHL_TRY
        as<Evaluator>(thisptr)->begin_capture();
        SHL_CATCH
    }
    SHL_FUNC Evaluator_EndCapture(void *thisptr, void **graph)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        IfNullRet(graph, SHL_E_POINTER);
        SHL_TRY
        *graph = as<Evaluator>(thisptr)->end_capture();
        SHL_CATCH
    }
    SHL_FUNC Evaluator_LaunchGraph(void *thisptr, void *graph)
    {
        return ev_call(thisptr, { graph }, [&](Evaluator &ev) { ev.launch_graph(static_cast<const Evaluator::Graph *>(graph)); });
    }
    SHL_FUNC Graph_Destroy(void *graph)
    {
        IfNullRet(graph, SHL_E_POINTER);
        delete static_cast<Evaluator::Graph *>(graph); // its scratch blocks return to the pool
        return SHL_S_OK;
    }
    SHL_FUNC Evaluator_SetTransparentCheck(void *thisptr, bool enabled)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        as<Evaluator>(thisptr)->set_transparent_check(enabled);
        return SHL_S_OK;
    }
    SHL_FUNC Evaluator_ContextUsingKeyswitching(void *thisptr, bool *using_keyswitching)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        IfNullRet(using_keyswitching, SHL_E_POINTER);
        *using_keyswitching = as<Evaluator>(thisptr)->context().using_keyswitching();
        return SHL_S_OK;
    }
    // destination := encrypted on the evaluator's stream (a pipeline with several evaluators / streams copies its inputs in
    // stream order; Ciphertext_Set works on the calling thread's stream)
    SHL_FUNC Evaluator_CopyTo(void *thisptr, void *encrypted, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &) { prepare_dest(encrypted, destination); });
    }
    SHL_FUNC Evaluator_Synchronize(void *thisptr)
    {
        return ev_call(thisptr, {}, [&](Evaluator &ev) { ev.synchronize(); });
    }
    SHL_FUNC Evaluator_Negate(void *thisptr, void *encrypted, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) { ev.negate_inplace(prepare_dest(encrypted, destination)); });
    }
    SHL_FUNC Evaluator_TransformToNTT2(void *thisptr, void *encrypted, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination },
                       [&](Evaluator &ev) { ev.transform_to_ntt_inplace(prepare_dest(encrypted, destination)); });
    }
    SHL_FUNC Evaluator_TransformFromNTT(void *thisptr, void *encrypted, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination },
                       [&](Evaluator &ev) { ev.transform_from_ntt_inplace(prepare_dest(encrypted, destination)); });
    }
    SHL_FUNC Evaluator_Square(void *thisptr, void *encrypted, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) { ev.square_inplace(prepare_dest(encrypted, destination)); });
    }
    SHL_FUNC Evaluator_ModSwitchToNext1(void *thisptr, void *encrypted, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, destination },
                       [&](Evaluator &ev) { ev.mod_switch_to_next_inplace(prepare_dest(encrypted, destination)); });
    }
    SHL_FUNC Evaluator_RescaleToNext(void *thisptr, void *encrypted, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, destination },
                       [&](Evaluator &ev) { ev.rescale_to_next_inplace(prepare_dest(encrypted, destination)); });
    }
    SHL_FUNC Evaluator_ModReduceToNext(void *thisptr, void *encrypted, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, destination },
                       [&](Evaluator &ev) { ev.mod_reduce_to_next_inplace(prepare_dest(encrypted, destination)); });
    }

    // ------------------------------------------------------------------ plaintext operands, many-operand forms
    SHL_FUNC Evaluator_AddPlain(void *thisptr, void *encrypted, void *plain, void *destination)
    {
        return ev_call(thisptr, { encrypted, plain, destination },
                       [&](Evaluator &ev) { ev.add_plain_inplace(prepare_dest(encrypted, destination), pt(plain)); });
    }
    SHL_FUNC Evaluator_SubPlain(void *thisptr, void *encrypted, void *plain, void *destination)
    {
        return ev_call(thisptr, { encrypted, plain, destination },
                       [&](Evaluator &ev) { ev.sub_plain_inplace(prepare_dest(encrypted, destination), pt(plain)); });
    }
    SHL_FUNC Evaluator_MultiplyPlain(void *thisptr, void *encrypted, void *plain, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, plain, destination },
                       [&](Evaluator &ev) { ev.multiply_plain_inplace(prepare_dest(encrypted, destination), pt(plain)); });
    }
    // one plaintext per item, raw device words (library extensions): no copy into the destination first - the host code shapes it
    SHL_FUNC Evaluator_AddPlainDevice(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t batch, bool plain_is_ntt, double scale,
                                      void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) {
            ev.add_plain_device(ct(encrypted), device_plain, (size_t)batch, plain_is_ntt, scale, ct(destination));
        });
    }
    SHL_FUNC Evaluator_SubPlainDevice(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t batch, bool plain_is_ntt, double scale,
                                      void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) {
            ev.sub_plain_device(ct(encrypted), device_plain, (size_t)batch, plain_is_ntt, scale, ct(destination));
        });
    }
    SHL_FUNC Evaluator_MultiplyPlainDevice(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t batch, bool plain_is_ntt,
                                           double scale, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) {
            ev.multiply_plain_device(ct(encrypted), device_plain, (size_t)batch, plain_is_ntt, scale, ct(destination));
        });
    }
    SHL_FUNC Evaluator_TransformPlainToNTTDevice(void *thisptr, const uint64_t *device_coefficients, uint64_t batch, uint64_t *parms_id,
                                                 uint64_t *device_words)
    {
        return ev_call(thisptr, { parms_id },
                       [&](Evaluator &ev) { ev.transform_plain_to_ntt_device(device_coefficients, (size_t)batch, parms_id, device_words); });
    }
    // sums over the items of a batch (library extensions): the destination is another handle, shaped by the host code
    SHL_FUNC Evaluator_SumItems(void *thisptr, void *encrypted, uint64_t group, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) { ev.sum_items(ct(encrypted), (size_t)group, ct(destination)); });
    }
    SHL_FUNC Evaluator_DotPlainDevice(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t batch, uint64_t group, double scale,
                                      void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) {
            ev.dot_plain_device(ct(encrypted), device_plain, (size_t)batch, (size_t)group, scale, ct(destination));
        });
    }
    SHL_FUNC Evaluator_DotItems(void *thisptr, void *encrypted1, void *encrypted2, uint64_t group, void *destination)
    {
        return ev_call(thisptr, { encrypted1, encrypted2, destination },
                       [&](Evaluator &ev) { ev.dot_items(ct(encrypted1), ct(encrypted2), (size_t)group, ct(destination)); });
    }
    // item maps (library extensions): a CSR list of item numbers in device memory, and the three reductions over the items it names
    SHL_FUNC ItemMap_Create(void *context, uint64_t rows, const uint64_t *row_offsets, const uint64_t *first_items, const uint64_t *second_items,
                            uint64_t first_batch, uint64_t second_batch, void **item_map)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(item_map, SHL_E_POINTER);
        SHL_TRY
        *item_map = new ItemMap(*as<Context>(context), rows, row_offsets, first_items, second_items, first_batch, second_batch);
        SHL_CATCH
    }
    SHL_FUNC ItemMap_Destroy(void *thisptr)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        SHL_TRY
        delete as<ItemMap>(thisptr);
        SHL_CATCH
    }
    SHL_FUNC ItemMap_Info(void *thisptr, uint64_t *rows, uint64_t *terms, uint64_t *longest_row, uint64_t *first_batch, uint64_t *second_batch)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        const ItemMap *m = as<ItemMap>(thisptr);
        if (rows)
            *rows = m->rows();
        if (terms)
            *terms = m->terms();
        if (longest_row)
            *longest_row = m->longest_row();
        if (first_batch)
            *first_batch = m->first_batch();
        if (second_batch)
            *second_batch = m->second_batch();
        return SHL_S_OK;
    }
    // Galois sets (library extension): R Galois elements, validated and uploaded once; one call rotates every item of a batch by all of them
    SHL_FUNC GaloisSet_Create(void *context, void *galois_keys, uint64_t count, const uint32_t *galois_elts, void **galois_set)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(galois_keys, SHL_E_POINTER);
        IfNullRet(galois_set, SHL_E_POINTER);
        SHL_TRY
        *galois_set = new GaloisSet(*as<Context>(context), keys(galois_keys), count, galois_elts, false);
        SHL_CATCH
    }
    SHL_FUNC GaloisSet_CreateFromSteps(void *context, void *galois_keys, uint64_t count, const int *steps, void **galois_set)
    {
        IfNullRet(context, SHL_E_POINTER);
        IfNullRet(galois_keys, SHL_E_POINTER);
        IfNullRet(galois_set, SHL_E_POINTER);
        SHL_TRY
        if (!steps)
            throw std::invalid_argument("steps is null");
        if (!count || count >= (uint64_t(1) << 32))
            throw std::invalid_argument("1 <= count < 2^32");
        Evaluator ev(*as<Context>(context));
        std::vector<uint32_t> elts;
        for (uint64_t r = 0; r < count; r++)
            elts.push_back(steps[r] ? ev.galois_elt_from_step(steps[r]) : 0); // a step of 0: the identity entry (a copy)
        *galois_set = new GaloisSet(*as<Context>(context), keys(galois_keys), count, elts.data(), true);
        SHL_CATCH
    }
    SHL_FUNC GaloisSet_Destroy(void *thisptr)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        SHL_TRY
        delete as<GaloisSet>(thisptr);
        SHL_CATCH
    }
    SHL_FUNC GaloisSet_Info(void *thisptr, uint64_t *count, uint64_t *identities, uint64_t *distinct, bool *register_order)
    {
        IfNullRet(thisptr, SHL_E_POINTER);
        const GaloisSet *s = as<GaloisSet>(thisptr);
        if (count)
            *count = s->count();
        if (identities)
            *identities = s->count() - s->switched();
        if (distinct)
            *distinct = s->distinct();
        if (register_order)
            *register_order = s->register_order();
        return SHL_S_OK;
    }
    SHL_FUNC Evaluator_ApplyGaloisSet(void *thisptr, void *encrypted, void *galois_set, void *destination)
    {
        return ev_call(thisptr, { encrypted, galois_set, destination },
                       [&](Evaluator &ev) { ev.apply_galois_set(ct(encrypted), *as<GaloisSet>(galois_set), ct(destination)); });
    }
    SHL_FUNC Evaluator_SumItemsMapped(void *thisptr, void *encrypted, void *item_map, void *destination)
    {
        return ev_call(thisptr, { encrypted, item_map, destination },
                       [&](Evaluator &ev) { ev.sum_items_mapped(ct(encrypted), *as<ItemMap>(item_map), ct(destination)); });
    }
    SHL_FUNC Evaluator_DotPlainMapped(void *thisptr, void *encrypted, const uint64_t *device_plain, uint64_t plain_count, void *item_map,
                                      double scale, void *destination)
    {
        return ev_call(thisptr, { encrypted, item_map, destination }, [&](Evaluator &ev) {
            ev.dot_plain_mapped(ct(encrypted), device_plain, (size_t)plain_count, *as<ItemMap>(item_map), scale, ct(destination));
        });
    }
    SHL_FUNC Evaluator_DotItemsMapped(void *thisptr, void *encrypted1, void *encrypted2, void *item_map, void *destination)
    {
        return ev_call(thisptr, { encrypted1, encrypted2, item_map, destination }, [&](Evaluator &ev) {
            ev.dot_items_mapped(ct(encrypted1), ct(encrypted2), *as<ItemMap>(item_map), ct(destination));
        });
    }
    // a sparse matrix of scalar weights over an item map (library extension); flags bit 2: the weights are signed 32-bit integers
    // and not [K] words each - Evaluator_MatMulScalarsItems' bit; no other bit is defined
    SHL_FUNC Evaluator_DotScalarsMapped(void *thisptr, void *encrypted, const void *device_weights, uint64_t weight_count, void *item_map,
                                        uint64_t flags, double scale, void *destination)
    {
        return ev_call(thisptr, { encrypted, item_map, destination }, [&](Evaluator &ev) {
            check_flags(flags, 4);
            ev.dot_scalars_mapped(ct(encrypted), device_weights, (size_t)weight_count, (flags & 4) != 0, *as<ItemMap>(item_map), scale,
                                  ct(destination));
        });
    }
    // scalar weights (library extensions): [count][K] words per scalar, and the dense matrix of them times a batch
    SHL_FUNC Evaluator_LiftScalars(void *thisptr, uint64_t count, const uint64_t *values_mod_t, uint64_t *parms_id, uint64_t *device_words)
    {
        return ev_call(thisptr, { parms_id }, [&](Evaluator &ev) { ev.lift_scalars((size_t)count, values_mod_t, parms_id, device_words); });
    }
    SHL_FUNC Evaluator_DotScalarsDevice(void *thisptr, void *encrypted, const uint64_t *device_scalars, uint64_t rows, uint64_t batch, double scale,
                                        void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) {
            ev.dot_scalars_device(ct(encrypted), device_scalars, (size_t)rows, (size_t)batch, scale, ct(destination));
        });
    }
    // ciphertext matrix x ciphertext matrix (library extension); flags bit 0: encrypted2 is stored [cols][inner]
    SHL_FUNC Evaluator_MatMulItems(void *thisptr, void *encrypted1, void *encrypted2, uint64_t rows, uint64_t inner, uint64_t cols, uint64_t flags,
                                   void *destination)
    {
        return ev_call(thisptr, { encrypted1, encrypted2, destination }, [&](Evaluator &ev) {
            check_flags(flags, 1);
            ev.matmul_items(ct(encrypted1), ct(encrypted2), (size_t)rows, (size_t)inner, (size_t)cols, (flags & 1) != 0, ct(destination));
        });
    }
    // plaintext matrix x ciphertext matrix (library extension); flags bit 0: encrypted is stored [cols][inner], bit 1: the result
    // is stored [cols][rows]
    SHL_FUNC Evaluator_MatMulPlainItems(void *thisptr, const uint64_t *device_plain, void *encrypted, uint64_t rows, uint64_t inner, uint64_t cols,
                                        uint64_t flags, double scale, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) {
            check_flags(flags, 3);
            ev.matmul_plain_items(device_plain, ct(encrypted), (size_t)rows, (size_t)inner, (size_t)cols, (flags & 1) != 0, (flags & 2) != 0, scale,
                                  ct(destination));
        });
    }
    // scalar weight matrix x ciphertext matrix (library extension); flags bits 0 and 1 as above, bit 2: the weights are signed 32-bit
    // integers and not [K] words each
    SHL_FUNC Evaluator_MatMulScalarsItems(void *thisptr, const void *device_weights, void *encrypted, uint64_t rows, uint64_t inner, uint64_t cols,
                                          uint64_t flags, double scale, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) {
            check_flags(flags, 7);
            ev.matmul_scalars_items(device_weights, (flags & 4) != 0, ct(encrypted), (size_t)rows, (size_t)inner, (size_t)cols, (flags & 1) != 0,
                                    (flags & 2) != 0, scale, ct(destination));
        });
    }
    // 2-D convolution of scalar weights over a grid of items (library extension); flags bit 0: the input is stored channel-last,
    // bit 1: the result is, bit 2: narrow weights
    SHL_FUNC Evaluator_Conv2dScalarsItems(void *thisptr, const void *device_weights, void *encrypted, const SHL_CONV2D *shape, uint64_t flags,
                                          double scale, void *destination)
    {
        return ev_call(thisptr, { encrypted, destination }, [&](Evaluator &ev) {
            if (!shape)
                throw std::invalid_argument("shape is null");
            check_flags(flags, 7);
            const Conv2dShape c{ shape->in_channels, shape->height,   shape->width,    shape->out_channels, shape->kernel_h,
                                 shape->kernel_w,    shape->stride_h, shape->stride_w, shape->pad_h,        shape->pad_w };
            ev.conv2d_scalars_items(device_weights, (flags & 4) != 0, ct(encrypted), c, (flags & 1) != 0, (flags & 2) != 0, scale,
                                    ct(destination));
        });
    }
    SHL_FUNC Evaluator_TransformToNTT1(void *thisptr, void *plain, uint64_t *parms_id, void *destination_ntt, void *)
    {
        return ev_call(thisptr, { plain, parms_id, destination_ntt },
                       [&](Evaluator &ev) { ev.transform_to_ntt_inplace(prepare_plain_dest(plain, destination_ntt), parms_id); });
    }
    SHL_FUNC Evaluator_ModSwitchToNext2(void *thisptr, void *plain, void *destination)
    {
        return ev_call(thisptr, { plain, destination }, [&](Evaluator &ev) { ev.mod_switch_to_next_inplace(prepare_plain_dest(plain, destination)); });
    }
    SHL_FUNC Evaluator_ModSwitchTo2(void *thisptr, void *plain, uint64_t *parms_id, void *destination)
    {
        return ev_call(thisptr, { plain, parms_id, destination },
                       [&](Evaluator &ev) { ev.mod_switch_to_inplace(prepare_plain_dest(plain, destination), parms_id); });
    }
    SHL_FUNC Evaluator_AddMany(void *thisptr, uint64_t count, void **encrypteds, void *destination)
    {
        return ev_call(thisptr, { encrypteds, destination }, [&](Evaluator &ev) { ev.add_many(ct_list(count, encrypteds), ct(destination)); });
    }
    SHL_FUNC Evaluator_MultiplyMany(void *thisptr, uint64_t count, void **encrypteds, void *relin_keys, void *destination, void *)
    {
        return ev_call(thisptr, { encrypteds, relin_keys, destination },
                       [&](Evaluator &ev) { ev.multiply_many(ct_list(count, encrypteds), keys(relin_keys), ct(destination)); });
    }
    SHL_FUNC Evaluator_Exponentiate(void *thisptr, void *encrypted, uint64_t exponent, void *relin_keys, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, relin_keys, destination },
                       [&](Evaluator &ev) { ev.exponentiate_inplace(prepare_dest(encrypted, destination), exponent, keys(relin_keys)); });
    }

    SHL_FUNC Evaluator_Add(void *thisptr, void *encrypted1, void *encrypted2, void *destination)
    {
        return ev_call(thisptr, { encrypted1, encrypted2, destination }, [&](Evaluator &ev) {
            if (encrypted2 == destination && encrypted1 != destination)
                ev.add_inplace(ct(destination), ct(encrypted1)); // evaluator.h add(): commutes
            else
                ev.add_inplace(prepare_dest(encrypted1, destination), ct(encrypted2));
        });
    }
    SHL_FUNC Evaluator_Sub(void *thisptr, void *encrypted1, void *encrypted2, void *destination)
    {
        return ev_call(thisptr, { encrypted1, encrypted2, destination }, [&](Evaluator &ev) {
            if (encrypted2 == destination && encrypted1 != destination)
            {
                // evaluator.h sub(): destination = e2 - e1, then negate
                ev.sub_inplace(ct(destination), ct(encrypted1));
                ev.negate_inplace(ct(destination));
            }
            else
                ev.sub_inplace(prepare_dest(encrypted1, destination), ct(encrypted2));
        });
    }
    SHL_FUNC Evaluator_Multiply(void *thisptr, void *encrypted1, void *encrypted2, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted1, encrypted2, destination }, [&](Evaluator &ev) {
            if (encrypted1 == encrypted2 && encrypted1 == destination)
                ev.multiply_inplace(ct(destination), ct(destination));
            else
                ev.multiply(ct(encrypted1), ct(encrypted2), ct(destination));
        });
    }
    SHL_FUNC Evaluator_Relinearize(void *thisptr, void *encrypted, void *relinKeys, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, relinKeys, destination },
                       [&](Evaluator &ev) { ev.relinearize_inplace(prepare_dest(encrypted, destination), keys(relinKeys)); });
    }
    SHL_FUNC Evaluator_SwitchKeyAccWords(void *thisptr, void *encrypted, uint64_t *words)
    {
        return ev_call(thisptr, { encrypted, words }, [&](Evaluator &ev) { *words = ev.switch_key_acc_words(ct(encrypted)); });
    }
    SHL_FUNC Evaluator_RelinearizePartial(void *thisptr, void *encrypted, void *relinKeys, uint64_t digit_first, uint64_t digit_count,
                                          uint64_t *device_acc)
    {
        return ev_call(thisptr, { encrypted, relinKeys, device_acc }, [&](Evaluator &ev) {
            ev.relinearize_partial(ct(encrypted), keys(relinKeys), (unsigned)digit_first, (unsigned)(digit_first + digit_count), device_acc);
        });
    }
    SHL_FUNC Evaluator_RelinearizeFinish(void *thisptr, void *encrypted, uint64_t *device_acc, uint64_t parts)
    {
        return ev_call(thisptr, { encrypted, device_acc }, [&](Evaluator &ev) { ev.relinearize_finish(ct(encrypted), device_acc, (unsigned)parts); });
    }
    SHL_FUNC Evaluator_ApplyGaloisPartial(void *thisptr, void *encrypted, uint32_t galois_elt, void *galoisKeys, uint64_t digit_first,
                                          uint64_t digit_count, uint64_t *device_acc)
    {
        return ev_call(thisptr, { encrypted, galoisKeys, device_acc }, [&](Evaluator &ev) {
            ev.apply_galois_partial(ct(encrypted), galois_elt, keys(galoisKeys), (unsigned)digit_first, (unsigned)(digit_first + digit_count),
                                    device_acc);
        });
    }
    SHL_FUNC Evaluator_ApplyGaloisFinish(void *thisptr, void *encrypted, uint64_t *device_acc, uint64_t parts)
    {
        return ev_call(thisptr, { encrypted, device_acc }, [&](Evaluator &ev) { ev.apply_galois_finish(ct(encrypted), device_acc, (unsigned)parts); });
    }
    // ------------------------------------------------------------------ communicator + digit-parallel forms with the exchange
    // inside the library (sealhip.h section 1c; comm.h)
    SHL_FUNC Comm_GetUniqueId(uint8_t *id128)
    {
        IfNullRet(id128, SHL_E_POINTER);
        SHL_TRY
        Comm::unique_id(id128);
        SHL_CATCH
    }
    SHL_FUNC Comm_RcclAvailable(bool *available)
    {
        IfNullRet(available, SHL_E_POINTER);
        SHL_TRY
        *available = Comm::rccl_available();
        SHL_CATCH
    }
    SHL_FUNC Comm_Create(const uint8_t *id128, int nranks, int rank, void **comm)
    {
        IfNullRet(comm, SHL_E_POINTER);
        SHL_TRY
        *comm = new Comm(id128, nranks, rank);
        SHL_CATCH
    }
    SHL_FUNC Comm_Destroy(void *comm)
    {
        IfNullRet(comm, SHL_E_POINTER);
        delete as<Comm>(comm);
        return SHL_S_OK;
    }
    SHL_FUNC Comm_Info(void *comm, int *nranks, int *rank, bool *loopback)
    {
        IfNullRet(comm, SHL_E_POINTER);
        SHL_TRY
        if (nranks)
            *nranks = as<Comm>(comm)->size();
        if (rank)
            *rank = as<Comm>(comm)->rank();
        if (loopback)
            *loopback = as<Comm>(comm)->loopback();
        SHL_CATCH
    }
    SHL_FUNC Comm_DigitRange(void *comm, uint64_t digits, uint64_t *first, uint64_t *count)
    {
        IfNullRet(comm, SHL_E_POINTER);
        IfNullRet(first, SHL_E_POINTER);
        IfNullRet(count, SHL_E_POINTER);
        SHL_TRY
        unsigned f, c;
        comm_split((unsigned)digits, (unsigned)as<Comm>(comm)->size(), (unsigned)as<Comm>(comm)->rank(), f, c);
        *first = f;
        *count = c;
        SHL_CATCH
    }
    SHL_FUNC Comm_AllReduceWords(void *comm, uint64_t *device_words, uint64_t count, void *hip_stream)
    {
        IfNullRet(comm, SHL_E_POINTER);
        IfNullRet(device_words, SHL_E_POINTER);
        SHL_TRY
        as<Comm>(comm)->all_reduce_sum(device_words, (size_t)count, (hipStream_t)hip_stream);
        SHL_CATCH
    }
    SHL_FUNC Comm_BroadcastWords(void *comm, uint64_t *device_words, uint64_t count, int root, void *hip_stream)
    {
        IfNullRet(comm, SHL_E_POINTER);
        IfNullRet(device_words, SHL_E_POINTER);
        SHL_TRY
        as<Comm>(comm)->broadcast(device_words, (size_t)count, root, (hipStream_t)hip_stream);
        SHL_CATCH
    }
    SHL_FUNC Evaluator_RelinearizeDigitParallel(void *thisptr, void *encrypted, void *relinKeys, void *comm, int exchange, void *destination)
    {
        return ev_call(thisptr, { encrypted, relinKeys, comm, destination }, [&](Evaluator &ev) {
            ev.relinearize_inplace(prepare_dest(encrypted, destination), keys(relinKeys), *as<Comm>(comm), exchange_of(exchange));
        });
    }
    SHL_FUNC Evaluator_ApplyGaloisDigitParallel(void *thisptr, void *encrypted, uint32_t galois_elt, void *galoisKeys, void *comm, int exchange,
                                                void *destination)
    {
        return ev_call(thisptr, { encrypted, galoisKeys, comm, destination }, [&](Evaluator &ev) {
            ev.apply_galois_inplace(prepare_dest(encrypted, destination), galois_elt, keys(galoisKeys), *as<Comm>(comm), exchange_of(exchange));
        });
    }
    SHL_FUNC Evaluator_RotateVectorDigitParallel(void *thisptr, void *encrypted, int steps, void *galoisKeys, void *comm, int exchange,
                                                 void *destination)
    {
        return ev_call(thisptr, { encrypted, galoisKeys, comm, destination }, [&](Evaluator &ev) {
            ev.rotate_vector_inplace(prepare_dest(encrypted, destination), steps, keys(galoisKeys), *as<Comm>(comm), exchange_of(exchange));
        });
    }
    SHL_FUNC Evaluator_BroadcastKeyDigits(void *thisptr, void *kswitch_keys, uint64_t index, uint64_t *device_staging, void *comm, int root)
    {
        return ev_call(thisptr, { kswitch_keys, device_staging, comm }, [&](Evaluator &ev) {
            ev.broadcast_key_digits(keys(kswitch_keys), (size_t)index, device_staging, *as<Comm>(comm), root);
        });
    }
    // the local phases of the reduce-scatter exchange (tests emulate the ranks in one process)
    SHL_FUNC Evaluator_SwitchKeySlots(void *thisptr, void *encrypted, uint64_t nranks, uint64_t *slots)
    {
        return ev_call(thisptr, { encrypted, slots }, [&](Evaluator &ev) { *slots = ev.switch_key_slots(ct(encrypted), (unsigned)nranks); });
    }
    SHL_FUNC Evaluator_SwitchKeyPackTargets(void *thisptr, void *encrypted, const uint64_t *device_acc, uint64_t nranks, uint64_t *device_send,
                                            uint64_t *device_special)
    {
        return ev_call(thisptr, { encrypted }, [&](Evaluator &ev) {
            ev.switch_key_pack_targets(ct(encrypted), device_acc, (unsigned)nranks, device_send, device_special);
        });
    }
    SHL_FUNC Evaluator_SwitchKeyFinishOwned(void *thisptr, void *encrypted, const uint64_t *device_recv, const uint64_t *device_special,
                                            uint64_t nranks, uint64_t rank, uint64_t *device_own)
    {
        return ev_call(thisptr, { encrypted }, [&](Evaluator &ev) {
            ev.switch_key_finish_owned(ct(encrypted), device_recv, device_special, (unsigned)nranks, (unsigned)rank, device_own);
        });
    }
    SHL_FUNC Evaluator_SwitchKeyAddGathered(void *thisptr, void *encrypted, const uint64_t *device_all, uint64_t nranks)
    {
        return ev_call(thisptr, { encrypted }, [&](Evaluator &ev) { ev.switch_key_add_gathered(ct(encrypted), device_all, (unsigned)nranks); });
    }
    SHL_FUNC Evaluator_ModSwitchTo1(void *thisptr, void *encrypted, uint64_t *parms_id, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, parms_id, destination },
                       [&](Evaluator &ev) { ev.mod_switch_to_inplace(prepare_dest(encrypted, destination), parms_id); });
    }
    SHL_FUNC Evaluator_RescaleTo(void *thisptr, void *encrypted, uint64_t *parms_id, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, parms_id, destination },
                       [&](Evaluator &ev) { ev.rescale_to_inplace(prepare_dest(encrypted, destination), parms_id); });
    }
    SHL_FUNC Evaluator_ModReduceTo(void *thisptr, void *encrypted, uint64_t *parms_id, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, parms_id, destination },
                       [&](Evaluator &ev) { ev.mod_reduce_to_inplace(prepare_dest(encrypted, destination), parms_id); });
    }
    SHL_FUNC Evaluator_ApplyGalois(void *thisptr, void *encrypted, uint32_t galois_elt, void *galoisKeys, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, galoisKeys, destination },
                       [&](Evaluator &ev) { ev.apply_galois(ct(encrypted), galois_elt, keys(galoisKeys), ct(destination)); });
    }
    SHL_FUNC Evaluator_RotateRows(void *thisptr, void *encrypted, int steps, void *galoisKeys, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, galoisKeys, destination },
                       [&](Evaluator &ev) { ev.rotate_rows(ct(encrypted), steps, keys(galoisKeys), ct(destination)); });
    }
    SHL_FUNC Evaluator_RotateColumns(void *thisptr, void *encrypted, void *galois_keys, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, galois_keys, destination },
                       [&](Evaluator &ev) { ev.rotate_columns(ct(encrypted), keys(galois_keys), ct(destination)); });
    }
    SHL_FUNC Evaluator_RotateVector(void *thisptr, void *encrypted, int steps, void *galoisKeys, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, galoisKeys, destination },
                       [&](Evaluator &ev) { ev.rotate_vector(ct(encrypted), steps, keys(galoisKeys), ct(destination)); });
    }
    SHL_FUNC Evaluator_ComplexConjugate(void *thisptr, void *encrypted, void *galoisKeys, void *destination, void *)
    {
        return ev_call(thisptr, { encrypted, galoisKeys, destination },
                       [&](Evaluator &ev) { ev.complex_conjugate(ct(encrypted), keys(galoisKeys), ct(destination)); });
    }
}
