/*
 * kfpos_ingest.h -- ranging ingest / epoch assembly for MANY tags in front of the batched core
 * (the step immediately before the hot path).
 *
 * Per tag this is PosGenerator's table logic, kept quirk for quirk:
 *   processRangingNow                src/kfpos/publishers/Posgenerator.cpp:201-281
 *   sendRangingMeasurementIfAvailable                              :155-198
 *   calculateTagLocationWithRangings                               :476-496
 *   timerRangingCallback (50 ms one-shot, MAX_TIME_TO_SEND_RANGING) :143-152, Posgenerator.h:77
 *   tag_reports_t                    src/kfpos/publishers/Posgenerator.h:78-105
 * i.e. ranges are floor()ed to integer millimetres (:213) and stored per 8-bit sequence number and
 * anchor column; a message with a NEW sequence number first flushes the previous sequence to the
 * estimator (:246-247); only column 0 of the new row is reset (:251-255 -- sic: columns 1..63 keep what
 * the same sequence number held 256 epochs ago unless a message overwrites them); errorEstimation is
 * stored on a same-sequence message only when > 0 (:241-243, :95); a flush does not clear anything, so
 * a timer flush followed by the next sequence number hands the same epoch to the estimator twice.
 *
 * What changes is the fan-out: the reference node drops every tag but one (:203) and its single timer
 * serves list index 0 (:148-150). Here every tag owns a row of the batch and its own 50 ms deadline, and
 * flushed epochs are handed to the GPU together, with the estimator's wall-clock timeLag computed per tag
 * and dt < 0 for the tags that have nothing in a round. The caller supplies time (seconds, monotonic) with
 * every event, as the adaptor does.
 *
 * Built for message rates, not for one tag (BASELINE configs[2]: 65 536 tags x 8 anchors x 20 Hz = 10.5 M
 * messages/s in front of a 40 us kernel):
 *   - tag and anchor ids resolve through flat open-addressing tables, the per-(tag, sequence) rows live in one
 *     allocation, count + ranges + errorEstimations of a row side by side; onRangingBatch() prefetches the
 *     rows of the messages a few places ahead, so the table's DRAM latency overlaps the work on the
 *     current message;
 *   - a flushed epoch is written ONCE, straight into the pinned, component-major slot the GPU's DMA engine
 *     reads (kfpos_slot_*): no per-epoch vectors, no row-major intermediate, no layout turn on the device; only
 *     a tag's second call within one round goes through a (re-used) overflow arena;
 *   - rounds are submitted asynchronously: while the GPU works on round r the CPU assembles round r + 1 in the
 *     next slot.
 *
 * The other sensor callbacks of PosGenerator (Posgenerator.cpp:99-141) are accepted per tag too (onImu,
 * onPX4Flow, onCompass, onMag): they queue behind that tag's pending ranging epochs, so each filter sees its
 * calls in arrival order, and a round hands every kind to the GPU in one call (the IMU slot kind for the 9-state
 * filter, kfpos_step_sensor for the planar one; the 6-state filter ignores them like the reference does).
 *
 * setSparseRounds(true): a round is assembled as a ROW LIST instead (kfpos_slot_submit_rows, kfpos_step_sensor_rows):
 * each call appends its row and one contiguous record, only the reporters' bytes cross the bus, and the GPU steps a
 * compact copy of them. Same filters, bit for bit; which mode is cheaper depends on the fraction of the bank that
 * reports per round.
 *
 * setDeltaRanges(true): whole-bank ranging rounds carry their ranges as 16-bit deltas (KFPOS_SLOT_RANGES_D16, kfpos_d16.h):
 * the round's slot is opened with kfpos_slot_delta and a flushed epoch is written as codes through kfpos_d16_put instead
 * of int32 ranges -- half the bytes of the largest array a round uploads; silent tags keep their stale codes (dt < 0:
 * not read). Same filters, bit for bit. Sparse rounds ignore the switch: row lists stay int32.
 */
#ifndef KFPOS_INGEST_H
#define KFPOS_INGEST_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "kfpos.h"

namespace kfpos_host {

/* gtec_msgs::Ranging as PosGenerator::newTOAMeasurement receives it, plus its arrival time */
struct RangingMsg {
    double now;             /* seconds, monotonic */
    int anchorId, tagId;
    double range;           /* millimetres; floor()ed on entry (Posgenerator.cpp:213) */
    double errorEstimation; /* m^2 */
    int seq;
};

/* int -> int, open addressing with linear probing: one probe for almost every lookup. erase() closes the gap it leaves
 * (backward-shift deletion: every entry of the cluster behind it moves up as far as its home slot allows), so the table
 * holds no tombstones and lookups stay as short after any number of erase / insert as right after build(). */
class FlatIdMap {
public:
    void build(const std::vector<int> &ids) {
        reserve(ids.size());
        for (size_t i = 0; i < ids.size(); ++i) insert(ids[i], (int)i); /* a repeated id keeps its last position, like std::map::operator[] did */
    }
    /* an empty table for up to n ids (load factor <= 1/2) */
    void reserve(size_t n) {
        size_t cap = 16;
        while (cap < 2 * n + 2) cap <<= 1;
        mask_ = cap - 1;
        key_.assign(cap, empty());
        val_.assign(cap, -1);
        size_ = 0;
        limit_ = n;
    }
    int find(int id) const {
        size_t p = hash(id);
        while (key_[p] != empty()) {
            if (key_[p] == id) return val_[p];
            p = (p + 1) & mask_;
        }
        return -1;
    }
    /* id -> value; an id already present gets the new value. At most the reserve()d number of ids. */
    void insert(int id, int value) {
        size_t p = hash(id);
        while (key_[p] != empty() && key_[p] != id) p = (p + 1) & mask_;
        if (key_[p] == empty()) {
            if (size_ >= limit_) throw std::length_error("FlatIdMap::insert: more ids than reserved");
            ++size_;
        }
        key_[p] = id;
        val_[p] = value;
    }
    /* true if the id was present */
    bool erase(int id) {
        size_t hole = hash(id);
        while (key_[hole] != empty() && key_[hole] != id) hole = (hole + 1) & mask_;
        if (key_[hole] == empty()) return false;
        for (size_t q = (hole + 1) & mask_; key_[q] != empty(); q = (q + 1) & mask_) {
            /* the entry at q may move into the hole if that is not in front of its home slot (distances along the probe
             * sequence, cyclic) */
            const size_t home = hash((int)key_[q]);
            if (((q - home) & mask_) >= ((q - hole) & mask_)) {
                key_[hole] = key_[q];
                val_[hole] = val_[q];
                hole = q;
            }
        }
        key_[hole] = empty();
        val_[hole] = -1;
        --size_;
        return true;
    }
    size_t size() const { return size_; }
    /* diagnostic (tests, tuning; not used by the ingest): slots looked at by find(id), 1 = found (or known absent) at
     * its home slot */
    int probes(int id) const {
        int n = 1;
        for (size_t p = hash(id); key_[p] != empty() && key_[p] != id; p = (p + 1) & mask_) ++n;
        return n;
    }

private:
    static int64_t empty() { return INT64_MIN; }
    size_t hash(int id) const { return ((uint64_t)(uint32_t)id * 0x9E3779B97F4A7C15ull >> 32) & mask_; }
    std::vector<int64_t> key_;
    std::vector<int> val_;
    size_t mask_ = 0, size_ = 0, limit_ = 0;
};

class BatchedRangingNode {
public:
    static constexpr double kMaxTimeToSendRanging = 0.05; /* MAX_TIME_TO_SEND_RANGING */

    /* tagIds: the tag id served by batch row t; handle: n_tags == tagIds.size(), anchors already set in
     * the same order as anchorIds (column a = anchorIds[a], the reference's _anchorIndexById). */
    BatchedRangingNode(kfpos_handle *h, const std::vector<int> &tagIds, const std::vector<int> &anchorIds)
        : h_(h), T_((int)tagIds.size()), A_((int)anchorIds.size()) {
        row_.build(tagIds);
        rowId_ = tagIds;
        bound_.assign(T_, 1);
        init(anchorIds);
    }
    /* nRows free rows (handle: n_tags == nRows): tags are admitted with bindRows() as they show up */
    BatchedRangingNode(kfpos_handle *h, int nRows, const std::vector<int> &anchorIds)
        : h_(h), T_(nRows), A_((int)anchorIds.size()) {
        row_.reserve(nRows);
        rowId_.assign(T_, 0);
        bound_.assign(T_, 0);
        init(anchorIds);
    }

    /* ---- tags that come and go: a row of the bank is reusable ----
     * Both calls are legal only while no call of any tag is pending, i.e. right after poll() returned and before the
     * next message (no round being assembled, nothing waiting for a later round); std::logic_error otherwise. There is
     * no queue for them: the caller picks the moment.
     *
     * releaseRows: the rows stop serving their tag ids. The ids leave the id map -- later messages for them are "not
     * one of ours", like any id this node was never told about --, and each row's table state goes back to its default:
     * its 256 sequence rows are initialised again on first use, the estimator clock restarts (the next tag's first call
     * has the first-call lag of 0.1 s), the 50 ms timer is disarmed; an epoch the tag still had open is dropped with it.
     * The filter itself is left as it is until the row is bound again. A row that is not bound: std::logic_error. */
    void releaseRows(const int *rows, int n) {
        requireIdle("releaseRows");
        for (int i = 0; i < n; ++i)
            if (rows[i] < 0 || rows[i] >= T_ || !bound_[rows[i]])
                throw std::logic_error("releaseRows: row " + std::to_string(rows[i]) + " is not bound");
        for (int i = 0; i < n; ++i) {
            const int r = rows[i];
            if (!bound_[r]) continue; /* listed twice */
            if (row_.find(rowId_[r]) == r) row_.erase(rowId_[r]);
            bound_[r] = 0;
            tags_[r] = Tag();
        }
    }
    /* bindRows: row rows[i] serves tag tagIds[i] from now on, its filter as a freshly created handle has it: ONE
     * kfpos_reset_tags for all n -- one wait on the pipeline per batch of admissions, not per tag --, then the ids enter
     * the map. initXyz: n x 3 start positions, or nullptr = the handle's kfpos_config.init_pos (it must be nullptr on a
     * handle that starts by ML initialisation). Rows must be free, ids must not be bound (nor listed twice):
     * std::logic_error, and nothing has changed. */
    void bindRows(const int *rows, const int *tagIds, int n, const double *initXyz) {
        requireIdle("bindRows");
        for (int i = 0; i < n; ++i) {
            if (rows[i] < 0 || rows[i] >= T_ || bound_[rows[i]])
                throw std::logic_error("bindRows: row " + std::to_string(rows[i]) + " is not free");
            if (row_.find(tagIds[i]) >= 0)
                throw std::logic_error("bindRows: tag id " + std::to_string(tagIds[i]) + " is already bound");
            for (int j = 0; j < i; ++j)
                if (rows[j] == rows[i] || tagIds[j] == tagIds[i])
                    throw std::logic_error("bindRows: row or tag id listed twice");
        }
        if (n <= 0) return;
        std::vector<int32_t> r(rows, rows + n);
        check(kfpos_reset_tags(h_, r.data(), n, initXyz), "kfpos_reset_tags");
        for (int i = 0; i < n; ++i) {
            row_.insert(tagIds[i], rows[i]);
            rowId_[rows[i]] = tagIds[i];
            bound_[rows[i]] = 1;
            tags_[rows[i]] = Tag();
        }
    }
    /* Sparse rounds (off by default): rounds go to the GPU as row lists -- see the head of this file. May be switched
     * whenever no call is pending (right after poll()); std::logic_error otherwise. */
    void setSparseRounds(bool on) {
        requireIdle("setSparseRounds");
        sparse_ = on;
    }
    bool sparseRounds() const { return sparse_; }
    /* Delta ranges (off by default): whole-bank ranging rounds go up as int16 codes -- see the head of this file. May be
     * switched whenever no call is pending, like setSparseRounds. */
    void setDeltaRanges(bool on) {
        requireIdle("setDeltaRanges");
        delta_ = on;
    }
    bool deltaRanges() const { return delta_; }
    /* Status words, if anybody wants them: sink(row, kind, status) for every estimator call made (kind 0 = ranging
     * epoch, KFPOS_SENSOR_* otherwise), in the order the calls were placed. A round's words are delivered when its slot
     * is taken again, or by deliverStatuses(), which waits for everything in flight. */
    using StatusSink = std::function<void(int row, int kind, uint32_t status)>;
    void setStatusSink(StatusSink sink) { sink_ = std::move(sink); }
    void deliverStatuses() {
        for (int s = 0; s < nSlots_; ++s) {
            if (flightKind_[s] < 0) continue;
            check(kfpos_slot_wait(h_, s), "kfpos_slot_wait");
            deliver(s);
        }
    }
    /* the row that serves tagId, -1 if none */
    int rowOf(int tagId) const { return row_.find(tagId); }
    bool bound(int row) const { return bound_[row] != 0; } /* diagnostic: does the row serve a tag at the moment */

    /* gtec_msgs::Ranging -> PosGenerator::newTOAMeasurement -> processRangingNow */
    void onRanging(double now, int anchorId, int tagId, double range, double errorEstimation, int seq) {
        const RangingMsg m = {now, anchorId, tagId, range, errorEstimation, seq};
        onRangingBatch(&m, 1);
    }

    /* A burst of ranging messages in arrival order (a network packet, a ROS queue drain). Same effect as calling
     * onRanging for each; the table rows of the messages kPrefetch places ahead are requested from memory early. */
    void onRangingBatch(const RangingMsg *m, size_t n) {
        constexpr size_t kPrefetch = 12;
        for (size_t i = 0; i < n; ++i) {
            if (i + kPrefetch < n) {
                const int r = row_.find(m[i + kPrefetch].tagId);
                if (r >= 0) {
                    __builtin_prefetch(&tags_[r], 1);
                    unsigned char *p = seqRow(r, m[i + kPrefetch].seq & 0xff);
                    __builtin_prefetch(p, 1);
                    __builtin_prefetch(p + 64, 1);
                }
            }
            ranging(m[i]);
        }
        messages_ += n;
    }

    /* sensor_msgs::Imu -> PosGenerator::newIMUMeasurement (Posgenerator.cpp:126-141) */
    void onImu(double now, int tagId, const double angVel[3], const double covAngVel[9], const double linAcc[3],
               const double covAcc[9]) {
        double d[24];
        for (int k = 0; k < 3; ++k) { d[k] = angVel[k]; d[12 + k] = linAcc[k]; }
        for (int k = 0; k < 9; ++k) { d[3 + k] = covAngVel[k]; d[15 + k] = covAcc[k]; }
        sensor(now, tagId, KFPOS_SENSOR_IMU, d, 24);
    }
    /* mavros_msgs::OpticalFlowRad -> newPX4FlowMeasurement, gated as Posgenerator.cpp:100 does */
    void onPX4Flow(double now, int tagId, double integratedX, double integratedY, double integratedZgyro,
                   double integrationTimeUs, int quality) {
        if (!(integrationTimeUs > 0 && quality > 0)) return;
        const double d[5] = {integratedX, integratedY, integratedZgyro, integrationTimeUs, (double)quality};
        sensor(now, tagId, KFPOS_SENSOR_PX4FLOW, d, 5);
    }
    /* std_msgs::Float64 -> newCompassMeasurement (:121-123) */
    void onCompass(double now, int tagId, double heading) { sensor(now, tagId, KFPOS_SENSOR_COMPASS, &heading, 1); }
    /* sensor_msgs::MagneticField -> newMAGMeasurement (:106-118) */
    void onMag(double now, int tagId, const double field[3]) { sensor(now, tagId, KFPOS_SENSOR_MAG, field, 3); }

    /* Advance time: fire the 50 ms deadlines that have passed (timerRangingCallback), then hand every
     * pending epoch to the GPU. Returns the number of estimator calls made (tag-epochs). The GPU may still be
     * working on them when this returns; every synchronous kfpos_* call (kfpos_get_pose_each, ...) waits first. */
    int poll(double now) {
        for (int t = 0; t < T_; ++t) {
            Tag &tg = tags_[t];
            if (tg.armed && tg.deadline <= now) {
                tg.armed = false; /* one-shot */
                flush(t, tg.deadline);
            }
        }
        return drain();
    }

    /* the tags' estimator clocks, for getPose extrapolation: seconds since each tag's last estimate */
    double sinceLastEstimate(int row, double now) const { return tags_[row].started ? now - tags_[row].last : 0.0; }
    bool started(int row) const { return tags_[row].started; }
    /* The publish tick of a sparse node: getPose for the n listed rows (the tags that reported since the last tick), each
     * extrapolated by "now minus my last estimate" (Posgenerator.cpp:541-548). pos n x 3, cov n x 9, vel n x 3, status
     * n, any of them NULL. What crosses the bus follows n (kfpos_get_pose_rows); like every synchronous call it first
     * waits for what poll() left in flight. Returns the KFPOS_* code; rows outside the bank are refused there. */
    int getPoseRows(const int *rows, int n, double now, double *pos, double *cov, double *vel, uint32_t *status) {
        std::vector<int32_t> list((size_t)(n > 0 ? n : 0));
        std::vector<double> ahead(list.size() ? list.size() : 1, 0.0);
        for (size_t i = 0; i < list.size(); ++i) {
            list[i] = rows[i];
            ahead[i] = (rows[i] >= 0 && rows[i] < T_) ? sinceLastEstimate(rows[i], now) : 0.0;
        }
        return kfpos_get_pose_rows(h_, list.data(), n, ahead.data(), n > 1 ? n : 1, pos, cov, vel, status);
    }
    int rows() const { return T_; }
    uint64_t messages() const { return messages_; }    /* ranging messages taken in so far */
    uint64_t overflowCalls() const { return overflowed_; } /* calls that had to wait for a later round */

private:
    struct Tag {
        double deadline = 0.0;
        double last = 0.0;    /* the estimator's mLastKFTimestamp */
        int seq = -1;         /* rangeSeq */
        bool armed = false;
        bool started = false; /* mLastKFTimestamp != min */
        bool live = false;    /* its rows of the table are initialised (initialiseTagList) */
    };
    struct Overflow { /* a call that found its tag already taken in the round being assembled */
        int row, kind;
        double lag;
        size_t off; /* ranging: A ints in ovInt_ and A doubles in ovDbl_; sensor: its sample in ovDbl_ */
    };

    void init(const std::vector<int> &anchorIds) {
        col_.build(anchorIds);
        tags_.resize(T_);
        real_ = kfpos_real_size(h_);
        dim_ = kfpos_state_dim(h_);
        nSlots_ = kfpos_slot_count(h_) < kMaxSlots ? kfpos_slot_count(h_) : kMaxSlots;
        /* one (tag, sequence) row: count, A ranges, A errorEstimations, padded to whole cache lines */
        rowBytes_ = ((sizeof(int32_t) * (1 + A_) + 7) & ~(size_t)7) + sizeof(double) * A_;
        rowBytes_ = (rowBytes_ + 63) & ~(size_t)63;
        errOff_ = (sizeof(int32_t) * (1 + A_) + 7) & ~(size_t)7;
        table_.reset(new unsigned char[(size_t)T_ * 256 * rowBytes_ + 64]); /* untouched until a tag speaks up */
        tableBase_ = (unsigned char *)(((uintptr_t)table_.get() + 63) & ~(uintptr_t)63);
        taken_.assign(T_, 0);
        for (int k = 0; k < 5; ++k) roundSlot_[k] = -1;
        for (int s = 0; s < kMaxSlots; ++s) flightKind_[s] = -1;
        if (dim_ == 8) { /* planar filter: its other four sensors go through the synchronous kfpos_step_sensor */
            for (int k = 1; k <= 4; ++k) sens_[k].assign((size_t)T_ * sensorWidth(k), 0.0);
            sensDt_.assign(T_, -1.0);
        }
    }
    void requireIdle(const char *who) const {
        if (roundCalls_ != 0 || !overflow_.empty())
            throw std::logic_error(std::string(who) + ": estimator calls are pending; call it right after poll()");
    }

    static int sensorWidth(int kind) {
        return kind == KFPOS_SENSOR_PX4FLOW ? 5 : kind == KFPOS_SENSOR_IMU ? 24 : kind == KFPOS_SENSOR_MAG ? 3 : 1;
    }
    static void check(int rc, const char *what) {
        if (rc != KFPOS_OK)
            throw std::runtime_error(std::string(what) + ": " + kfpos_strerror(rc) + " " + kfpos_last_error());
    }
    unsigned char *seqRow(int row, int s) const { return tableBase_ + ((size_t)row * 256 + s) * rowBytes_; }
    static int32_t &count(unsigned char *p) { return *(int32_t *)p; }
    static int32_t *values(unsigned char *p) { return (int32_t *)p + 1; }
    double *errs(unsigned char *p) const { return (double *)(p + errOff_); }

    void ranging(const RangingMsg &m) {
        const int r = row_.find(m.tagId);
        if (r < 0) return; /* not one of ours (Posgenerator.cpp:203) */
        const int a = col_.find(m.anchorId);
        if (a < 0) return;
        Tag &tg = tags_[r];
        if (!tg.live) { /* initialiseTagList, Posgenerator.cpp:499-507 */
            for (int s = 0; s < 256; ++s) {
                unsigned char *p = seqRow(r, s);
                count(p) = 0;
                for (int k = 0; k < A_; ++k) { values(p)[k] = -1; errs(p)[k] = 0.0; }
            }
            tg.seq = -1;
            tg.live = true;
        }
        if (tg.armed && tg.deadline <= m.now) { /* this tag's 50 ms timer fired before the message arrived */
            tg.armed = false;
            flush(r, tg.deadline);
        }
        const int32_t mm = (int32_t)std::floor(m.range); /* :213 */
        const int s = m.seq & 0xff;
        unsigned char *p = seqRow(r, s);
        if (tg.seq == s) {
            count(p)++;
            values(p)[a] = mm;
            if (m.errorEstimation > 0.0) errs(p)[a] = m.errorEstimation;
        } else {
            flush(r, m.now); /* :246-247 */
            values(p)[0] = -1; /* sic: column 0 only, :251-255 */
            errs(p)[0] = 0.0;
            count(p) = 1;
            tg.seq = s;
            values(p)[a] = mm;
            errs(p)[a] = m.errorEstimation;
        }
        tg.deadline = m.now + kMaxTimeToSendRanging; /* timerRanging.stop(); start(); :274-277 */
        tg.armed = true;
    }

    /* every estimator call reads the filter's clock on entry (KalmanFilterTOA.cpp:78-88): calls of one tag reach
     * here in arrival order, so its timeLag can be settled now */
    double lagOf(Tag &tg, double time) {
        const double lag = tg.started ? time - tg.last : 0.1;
        tg.last = time;
        tg.started = true;
        return lag;
    }

    void sensor(double now, int tagId, int kind, const double *data, int n) {
        const int r = row_.find(tagId);
        if (r < 0) return;
        /* the empty virtuals of PositionEstimationAlgorithm.h:26-35 do not touch the filter, nor its clock */
        if (!(dim_ == 8 || (dim_ == 9 && kind == KFPOS_SENSOR_IMU))) return;
        Tag &tg = tags_[r];
        if (tg.armed && tg.deadline <= now) { /* the ranging timer fired first */
            tg.armed = false;
            flush(r, tg.deadline);
        }
        const double lag = lagOf(tg, now);
        if (!taken_[r]) {
            place(r, kind, lag, nullptr, nullptr, data);
        } else {
            Overflow o = {r, kind, lag, ovDbl_.size()};
            ovDbl_.insert(ovDbl_.end(), data, data + n);
            overflow_.push_back(o);
            ++overflowed_;
        }
    }

    /* sendRangingMeasurementIfAvailable (:155-198): the current sequence row goes to the estimator */
    void flush(int row, double time) {
        Tag &tg = tags_[row];
        if (tg.seq == -1) return;
        unsigned char *p = seqRow(row, tg.seq);
        if (count(p) < 1) return;
        tg.armed = false; /* timerRanging.stop(), :172 */
        const double lag = lagOf(tg, time);
        if (!taken_[row]) {
            place(row, 0, lag, values(p), errs(p), nullptr);
        } else { /* a second epoch of this tag before the round left: keep a snapshot for the next round */
            const Overflow o = {row, 0, lag, ovDbl_.size()};
            ovIntOff_.push_back(ovInt_.size());
            ovInt_.insert(ovInt_.end(), values(p), values(p) + A_);
            ovDbl_.insert(ovDbl_.end(), errs(p), errs(p) + A_);
            overflow_.push_back(o);
            ++overflowed_;
        }
    }

    /* the slot (pinned; component-major, or in sparse mode row-major per listed tag) that collects this round's calls
     * of `kind` */
    int slotFor(int kind) {
        if (roundSlot_[kind] < 0) {
            const int s = nextSlot_++ % nSlots_;
            if (sparse_) { /* no dt = -1 fill, nothing to undo: the list says who is in the round */
                check(kfpos_slot_acquire_rows(h_, s, &rslot_[s]), "kfpos_slot_acquire_rows"); /* waits for its previous round */
                deliver(s);
                rowsN_[s] = 0;
                slotDelta_[s] = false;
                slotInit_[s] = false; /* its dt array no longer holds -1 everywhere */
            } else {
                check(kfpos_slot_acquire(h_, s, &slot_[s]), "kfpos_slot_acquire"); /* waits for its previous round */
                deliver(s);
                if (!slotInit_[s]) {
                    for (int t = 0; t < T_; ++t) slot_[s].dt[t] = -1.0;
                    slotInit_[s] = true;
                } else {
                    for (int t : written_[s]) slot_[s].dt[t] = -1.0;
                }
                slotDelta_[s] = kind == 0 && delta_;
                if (slotDelta_[s]) check(kfpos_slot_delta(h_, s, &dslot_), "kfpos_slot_delta"); /* one ranging round is assembled at a time */
            }
            written_[s].clear();
            roundSlot_[kind] = s;
        }
        return roundSlot_[kind];
    }
    /* the status words of the round slot s carried last (it has completed) */
    void deliver(int s) {
        if (flightKind_[s] < 0) return;
        if (sink_) {
            if (flightSparse_[s])
                for (int i = 0; i < rowsN_[s]; ++i) sink_(rslot_[s].rows[i], flightKind_[s], rslot_[s].status[i]);
            else
                for (int t : written_[s]) sink_(t, flightKind_[s], slot_[s].status[t]);
        }
        flightKind_[s] = -1;
    }

    /* one call of one tag into the round being assembled */
    void place(int row, int kind, double lag, const int32_t *mm, const double *err, const double *sample) {
        taken_[row] = 1;
        touched_.push_back(row);
        ++roundCalls_;
        const size_t T = (size_t)T_;
        if (sparse_ && (kind == 0 || dim_ == 9)) { /* append the row and ONE contiguous record */
            const int s = slotFor(kind == 0 ? 0 : KFPOS_SENSOR_IMU);
            kfpos_rows_slot &sl = rslot_[s];
            const size_t i = (size_t)rowsN_[s]++;
            sl.rows[i] = row;
            sl.dt[i] = lag;
            if (kind == 0) {
                int32_t *r = sl.range_mm + i * A_;
                for (int a = 0; a < A_; ++a) r[a] = mm[a] > 0 ? mm[a] : 0; /* only entries > 0 (:483) */
                if (real_ == 4) {
                    float *e = (float *)sl.err_est + i * A_;
                    for (int a = 0; a < A_; ++a) e[a] = (float)err[a];
                } else {
                    std::memcpy((double *)sl.err_est + i * A_, err, sizeof(double) * A_);
                }
            } else if (real_ == 4) {
                float *ac = (float *)sl.accel + i * 3, *cv = (float *)sl.cov + i * 9;
                for (int k = 0; k < 3; ++k) ac[k] = (float)sample[12 + k];
                for (int k = 0; k < 9; ++k) cv[k] = (float)sample[15 + k];
            } else {
                std::memcpy((double *)sl.accel + i * 3, sample + 12, sizeof(double) * 3);
                std::memcpy((double *)sl.cov + i * 9, sample + 15, sizeof(double) * 9);
            }
        } else if (kind == 0) {
            const int s = slotFor(0);
            kfpos_epoch_slot &sl = slot_[s];
            if (slotDelta_[s]) { /* a tag is placed once per round: every element is put at most once; <= 0 is ABSENT */
                for (int a = 0; a < A_; ++a)
                    if (kfpos_d16_put(&dslot_, (int64_t)a * T_ + row, mm[a])) throw std::logic_error("kfpos_d16_put: the escape list is full");
            } else {
                for (int a = 0; a < A_; ++a) sl.range_mm[(size_t)a * T + row] = mm[a] > 0 ? mm[a] : 0; /* only entries > 0 (:483) */
            }
            if (real_ == 4) {
                float *e = (float *)sl.err_est;
                for (int a = 0; a < A_; ++a) e[(size_t)a * T + row] = (float)err[a];
            } else {
                double *e = (double *)sl.err_est;
                for (int a = 0; a < A_; ++a) e[(size_t)a * T + row] = err[a];
            }
            sl.dt[row] = lag;
            written_[roundSlot_[0]].push_back(row);
        } else if (dim_ == 9) { /* KalmanFilterTOAIMU::newIMUMeasurement: acceleration + its covariance */
            kfpos_epoch_slot &sl = slot_[slotFor(KFPOS_SENSOR_IMU)];
            if (real_ == 4) {
                float *ac = (float *)sl.accel, *cv = (float *)sl.cov;
                for (int k = 0; k < 3; ++k) ac[(size_t)k * T + row] = (float)sample[12 + k];
                for (int k = 0; k < 9; ++k) cv[(size_t)k * T + row] = (float)sample[15 + k];
            } else {
                double *ac = (double *)sl.accel, *cv = (double *)sl.cov;
                for (int k = 0; k < 3; ++k) ac[(size_t)k * T + row] = sample[12 + k];
                for (int k = 0; k < 9; ++k) cv[(size_t)k * T + row] = sample[15 + k];
            }
            sl.dt[row] = lag;
            written_[roundSlot_[KFPOS_SENSOR_IMU]].push_back(row);
        } else { /* planar filter: the sample as the reference callback passes it; sparse: one record per listed tag */
            const int C = sensorWidth(kind);
            const size_t at = sparse_ ? sensRows_[kind].size() : (size_t)row;
            std::memcpy(&sens_[kind][at * C], sample, sizeof(double) * C);
            if (sensRows_[kind].empty()) sensKinds_.push_back(kind);
            sensRows_[kind].push_back(row);
            sensLag_[kind].push_back(lag);
        }
    }

    /* hand the assembled round to the GPU: one submission per kind present */
    void submitRound() {
        static const int kSlotKind[2][2] = {{0, KFPOS_SLOT_TOA}, {KFPOS_SENSOR_IMU, KFPOS_SLOT_IMU}};
        for (const auto &k : kSlotKind) {
            const int s = roundSlot_[k[0]];
            if (s < 0) continue;
            int flags = k[1] | KFPOS_SLOT_DT_PER_TAG | KFPOS_SLOT_NO_POSE;
            if (!sparse_ && k[0] == 0 && slotDelta_[s]) {
                sortEscapes();
                flags |= KFPOS_SLOT_RANGES_D16;
            }
            if (sparse_) check(kfpos_slot_submit_rows(h_, s, flags, rowsN_[s], 0.0), "kfpos_slot_submit_rows");
            else check(kfpos_slot_submit(h_, s, flags, 0.0), "kfpos_slot_submit");
            flightKind_[s] = k[0];
            flightSparse_[s] = sparse_;
            roundSlot_[k[0]] = -1;
        }
        for (int kind : sensKinds_) { /* planar sensors: synchronous (the call waits for the slots first) */
            const std::vector<int> &rows = sensRows_[kind];
            const int n = (int)rows.size();
            uint32_t *st = nullptr;
            if (sink_) {
                sensSt_.resize((size_t)T_);
                st = sensSt_.data();
            }
            if (sparse_) { /* no [T x C] staging: the samples lie one record per listed tag */
                check(kfpos_step_sensor_rows(h_, rows.data(), n, kind, sens_[kind].data(), sensLag_[kind].data(), n, st),
                      "kfpos_step_sensor_rows");
            } else {
                for (int i = 0; i < n; ++i) sensDt_[rows[i]] = sensLag_[kind][i];
                check(kfpos_step_sensor(h_, kind, sens_[kind].data(), sensDt_.data(), T_, st), "kfpos_step_sensor");
                for (int r : rows) sensDt_[r] = -1.0;
            }
            if (sink_)
                for (int i = 0; i < n; ++i) sink_(rows[i], kind, st[sparse_ ? i : rows[i]]);
            sensRows_[kind].clear();
            sensLag_[kind].clear();
        }
        sensKinds_.clear();
        for (int r : touched_) taken_[r] = 0;
        touched_.clear();
    }

    /* tags are placed in arrival order, the escape list of a D16 round ascends by flat index: put it in order */
    void sortEscapes() {
        const int32_t n = *dslot_.n_esc;
        int32_t *e = dslot_.esc;
        bool sorted = true;
        for (int32_t k = 1; k < n && sorted; ++k) sorted = e[2 * k] > e[2 * (k - 1)];
        if (sorted) return;
        escKeys_.resize((size_t)n);
        for (int32_t k = 0; k < n; ++k) escKeys_[k] = ((int64_t)e[2 * k] << 32) | (uint32_t)e[2 * k + 1];
        std::sort(escKeys_.begin(), escKeys_.end());
        for (int32_t k = 0; k < n; ++k) {
            e[2 * k] = (int32_t)(escKeys_[k] >> 32);
            e[2 * k + 1] = (int32_t)(uint32_t)escKeys_[k];
        }
    }

    /* A round takes at most one pending call per tag, in arrival order, and makes one submission per kind
     * present (tags without a call of that kind carry dt < 0). Tags are independent, so the order of the kinds
     * inside a round does not matter. The first round has been assembled in place as the calls came in; what did
     * not fit (a tag's second call) follows in further rounds. */
    int drain() {
        int calls = roundCalls_;
        submitRound();
        while (!overflow_.empty()) {
            std::vector<Overflow> rest;
            std::vector<size_t> restInt;
            size_t iInt = 0;
            for (const Overflow &o : overflow_) {
                const bool ranging = o.kind == 0;
                const size_t intOff = ranging ? ovIntOff_[iInt++] : 0;
                if (taken_[o.row]) {
                    rest.push_back(o);
                    if (ranging) restInt.push_back(intOff);
                    continue;
                }
                if (ranging) place(o.row, 0, o.lag, &ovInt_[intOff], &ovDbl_[o.off], nullptr);
                else place(o.row, o.kind, o.lag, nullptr, nullptr, &ovDbl_[o.off]);
            }
            overflow_.swap(rest);
            ovIntOff_.swap(restInt);
            calls = roundCalls_;
            submitRound();
        }
        ovInt_.clear();
        ovDbl_.clear();
        ovIntOff_.clear();
        roundCalls_ = 0;
        return calls;
    }

    kfpos_handle *h_;
    int T_, A_, real_ = 8, dim_ = 6;
    FlatIdMap row_, col_;
    std::vector<int> rowId_;           /* the tag id a bound row serves */
    std::vector<unsigned char> bound_; /* 0 = free row */
    std::vector<Tag> tags_;
    std::unique_ptr<unsigned char[]> table_;
    unsigned char *tableBase_ = nullptr;
    size_t rowBytes_ = 0, errOff_ = 0;
    /* the round being assembled */
    std::vector<unsigned char> taken_;
    std::vector<int> touched_;
    int roundCalls_ = 0;
    static constexpr int kMaxSlots = 8;
    int nSlots_ = 2;
    kfpos_epoch_slot slot_[kMaxSlots];
    /* sparse rounds: the same slots as row lists, and how many rows the round in each holds */
    static_assert(sizeof(int) == sizeof(int32_t), "row lists are int32_t");
    bool sparse_ = false;
    /* delta ranges: is the ranging round in a slot a D16 round, and the one that is open */
    bool delta_ = false, slotDelta_[kMaxSlots] = {false};
    kfpos_delta_slot dslot_ = {};
    std::vector<int64_t> escKeys_;
    kfpos_rows_slot rslot_[kMaxSlots];
    int rowsN_[kMaxSlots] = {0};
    /* what each slot has in flight (kind, -1 = nothing to deliver; assembled as a row list?) and who listens */
    int flightKind_[kMaxSlots];
    bool flightSparse_[kMaxSlots] = {false};
    StatusSink sink_;
    std::vector<uint32_t> sensSt_;
    bool slotInit_[kMaxSlots] = {false};
    std::vector<int> written_[kMaxSlots];
    int roundSlot_[5];
    int nextSlot_ = 0;
    std::vector<double> sens_[5], sensLag_[5], sensDt_;
    std::vector<int> sensRows_[5], sensKinds_;
    /* calls waiting for a later round */
    std::vector<Overflow> overflow_;
    std::vector<int32_t> ovInt_;
    std::vector<double> ovDbl_;
    std::vector<size_t> ovIntOff_;
    uint64_t messages_ = 0, overflowed_ = 0;
};

} // namespace kfpos_host
#endif
