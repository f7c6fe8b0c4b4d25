// The items of mask_parts.h on the device, for the kernels of mask_parts.hip and contours.hip: MpItemsDev owns the six uploads, view() is
// what a kernel's argument struct starts with.  For hipcc only (DevBuf is common.h's); mask_parts.h stays plain C++.
#pragma once
#include "common.h"
#include "mask_parts.h"

namespace amp {

struct MpItemsView {
    const unsigned int *S, *E, *col;
    const unsigned char* T;
    const MpMask* masks;
    const unsigned long long* first;             // [n + 1], in items
    int n;
    unsigned int R;                              // items
};
struct MpItemsDev {
    DevBuf S, E, T, col, first, masks;
    int n = 0;
    unsigned int R = 0;
    int upload(amp_ctx* ctx, const MpItems& it) {
        n = (int)it.m.size(); R = (unsigned int)it.S.size();
        AMP_TRY_STATUS(dev_upload(ctx, S, it.S));
        AMP_TRY_STATUS(dev_upload(ctx, E, it.E));
        AMP_TRY_STATUS(dev_upload(ctx, T, it.T));
        AMP_TRY_STATUS(dev_upload(ctx, col, it.col));
        AMP_TRY_STATUS(dev_upload(ctx, first, it.first));
        return dev_upload(ctx, masks, it.m);
    }
    MpItemsView view() const {
        return MpItemsView{S.as<unsigned int>(), E.as<unsigned int>(), col.as<unsigned int>(), T.as<unsigned char>(), masks.as<MpMask>(),
                           first.as<unsigned long long>(), n, R};
    }
};

}  // namespace amp
