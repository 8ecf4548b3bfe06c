// The compiled AIRs, listed once: the prover (vx_stark.hip) and the host verifier (vx_verify.hip) each expand this list into
// their own descriptor table, so an AIR added or resized here exists on both sides or on neither.  Order is irrelevant: both
// look an AIR up by its ID.  The oracle (oracle/stark_ref.py) keeps its own registry on purpose.
#pragma once
#include "air.cuh"
#include "air_blake.cuh"
#include "air_ed.cuh"
#include "air_epoch.cuh"
#include "air_fri_combine.cuh"
#include "air_fri_fold.cuh"
#include "air_leaf_noop.cuh"
#include "air_leaf_sponge.cuh"
#include "air_merkle_open.cuh"
#include "air_sha.cuh"
#include "air_sha512.cuh"
#include "air_sha_tree.cuh"
#include "air_transcript.cuh"
#include "vx_internal.h"

template <class... Airs>
struct AirList {};
using VxAirs = AirList<ShaAir, BlakeAir, FibAir, MixAir, LookupAir, ShaTreeAir256, ShaTreeAir512, ShaTreeAir16, EdAir17, EdAir16, Sha512Air16, Sha512Air10, Sha512Air15,
                       EpochEndAir, MerkleOpenAir, LeafSpongeAir, FriFoldAir, MerkleOpenSetAir, LeafSpongeSetAir, FriCombineAir, LeafNoopAir, TranscriptAir>;

template <class... Airs>
constexpr bool air_list_ok(AirList<Airs...>) {
    const int ids[] = {Airs::ID...};
    for (size_t i = 0; i < sizeof...(Airs); ++i)
        for (size_t j = 0; j < i; ++j)
            if (ids[i] == ids[j]) return false;
    // ids from VX_AIR_USER_BASE on belong to registered programs; an auxiliary round exactly where a generator exists; challenges
    // and published values fit the prover's fixed arrays
    return ((Airs::ID < VX_AIR_USER_BASE && (Airs::AUX > 0) == (gen_aux_fn(Airs::gen_aux) != nullptr) && Airs::CHAL <= 8 && 2 * Airs::AUXPUB <= 8) && ...);
}
static_assert(air_list_ok(VxAirs{}), "air_list.h: AIR ids must be distinct and below VX_AIR_USER_BASE, an AIR has a gen_aux exactly when AUX > 0, CHAL <= 8, 2 AUXPUB <= 8");
