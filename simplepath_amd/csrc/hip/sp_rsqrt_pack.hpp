// sp_rsqrt_pack.hpp -- the RSQRTSS table as the device holds it: RSQ_HDR header words
// {bits, zero_result, denorm_result, pack_shift, pack_hi, 0, 0, 0} followed by the entries
// (sp_device.hpp, sp_path.hpp Rsq).  Host code only; used by the scene upload and by
// tests/cpp/device_units.hip, so the unit tests read exactly the words a render kernel reads.
#pragma once
#include "sp_device.hpp"
#include <cstring>
#include <vector>

namespace spd {

// Entries become 16-bit device entries when `pack` is set and every entry has the same sign and
// exponent and at least 7 trailing zero mantissa bits (Intel and AMD hosts alike: exponent 126, 12
// significant bits): half the LDS each shading block copies it into (sp_math.h).  Otherwise, and
// with pack off (comparison), the entries follow the header as 32-bit words.
inline std::vector<uint32_t> rsqrt_device_words(const uint32_t* entries, size_t count, int32_t bits, uint32_t zero_result,
                                                uint32_t denorm_result, bool pack)
{
    int      rs_shift = 23;
    uint32_t rs_hi    = entries[0] & 0xff800000u;
    for (size_t i = 0; i < count; ++i) {
        const uint32_t e = entries[i];
        if ((e & 0xff800000u) != rs_hi) {
            rs_shift = 0;
            break;
        }
        while (rs_shift > 0 && (e & ((1u << rs_shift) - 1u))) --rs_shift;
    }
    if (!pack) rs_shift = 0; // 32-bit entries (comparison)
    if (rs_shift < 7) rs_shift = 0;
    const uint32_t hdr[RSQ_HDR] = { (uint32_t)bits, zero_result, denorm_result, (uint32_t)rs_shift,
                                    rs_shift ? rs_hi : 0u, 0u, 0u, 0u };
    std::vector<uint32_t> words(hdr, hdr + RSQ_HDR);
    if (rs_shift) {
        std::vector<uint16_t> packed(count);
        for (size_t i = 0; i < count; ++i) packed[i] = (uint16_t)((entries[i] & 0x7fffffu) >> rs_shift);
        words.resize(RSQ_HDR + (count + 1) / 2, 0u);
        std::memcpy(words.data() + RSQ_HDR, packed.data(), count * sizeof(uint16_t));
    } else {
        words.insert(words.end(), entries, entries + count);
    }
    return words;
}

} // namespace spd
