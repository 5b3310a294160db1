/*
 * kfpos_owned.h -- the owner of one resource of the handle or the communicator: a raw handle (a device pointer, a pinned
 * host pointer, an event, a stream) and the function that gives it back. Move-only; converts to the raw handle, so code
 * that reads h->d_pos does not know about it; null is never released. No HIP header: kfpos_internal.h names the four
 * aliases, tests/policy/policy_driver.cpp counts releases with stand-ins.
 */
#ifndef KFPOS_OWNED_H
#define KFPOS_OWNED_H

namespace kfpos_owned {

template <class T, auto Release>
class Owned {
    T p_ = T();

  public:
    Owned() = default;
    explicit Owned(T p) : p_(p) {}
    Owned(Owned &&o) noexcept : p_(o.release()) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) reset(o.release());
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }

    operator T() const { return p_; }
    /* gives back what it holds, then holds p */
    void reset(T p = T()) {
        const T old = p_;
        p_ = p;
        if (old) (void)Release(old);
    }
    /* hands what it holds to the caller, who owns it from here on */
    T release() {
        const T p = p_;
        p_ = T();
        return p;
    }
    /* where an allocating call writes its result (hipMalloc((void **)p.out(), n)): what was held is given back first */
    T *out() {
        reset();
        return &p_;
    }
};

} // namespace kfpos_owned
#endif /* KFPOS_OWNED_H */
